// Latent-space and loss kernels of the training step: reparameterisation + per-dim KL
// (vae.py:52-71, losses.py:452-480), reconstruction likelihoods (losses.py:394-449), the
// beta-TCVAE minibatch estimator and its analytic gradient (losses.py:523-544, math.py:8-73),
// FactorVAE permute_dims / discriminator losses (losses.py:261-265,293-295,483-508) and the
// scalar epilogue of the loss plugins.  All reductions are fixed-order (deterministic).
#include "common.h"

namespace dvae {

// ---- reparam + KL ----------------------------------------------------------------------------
// elementwise part over B*D threads; the per-dim KL sums go through per-workgroup partials
// ([64][16] floats, fixed order) and a one-wave finishing kernel
#define RK_BLOCKS 64
__global__ __launch_bounds__(256) void k_reparam_kl_fwd(const float* __restrict__ ml, const float* __restrict__ eps,
                                                        float* __restrict__ mu, float* __restrict__ logvar,
                                                        float* __restrict__ z, float* __restrict__ kl_part, int B, int D) {
  __shared__ float red[4][16];
  const int tid = threadIdx.x;
  float kl[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) kl[d] = 0.f;
  for (int b = blockIdx.x * 256 + tid; b < B; b += gridDim.x * 256) {
#pragma unroll
    for (int d = 0; d < 16; ++d) {
      if (d < D) {
        const float m = ml[(long)b * 2 * D + 2 * d], lv = ml[(long)b * 2 * D + 2 * d + 1];
        mu[(long)b * D + d] = m;
        logvar[(long)b * D + d] = lv;
        float zz = m;
        if (eps) zz = m + expf(0.5f * lv) * eps[(long)b * D + d];
        z[(long)b * D + d] = zz;
        kl[d] += kl_elem(m, lv);
      }
    }
  }
  if (!kl_part) return;
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    float v = wave_sum(kl[d]);
    if (lane == 0) red[wv][d] = v;
  }
  __syncthreads();
  if (tid < 16) kl_part[blockIdx.x * 16 + tid] = block_sum4_read(red, tid);
}

// fixed-order sum of `nblk` per-workgroup KL partial blocks ([nblk][16] floats) by a 256-thread workgroup: thread t adds
// the blocks g = t/16, t/16 + 16, ... of dimension t%16, then 16 threads add the 16 strided sums.  Returns the total in
// threads 0..15 (dimension = thread index); `klred` = 256 floats of LDS.  The order depends on nblk only, so every
// consumer of the same partials (the finishing kernel, the one-launch loss epilogue) produces the same bits.
__device__ __forceinline__ float kl_blocks_sum(const float* __restrict__ part, int nblk, float* klred) {
  const int tid = threadIdx.x;
  const int d = tid & 15, g0 = tid >> 4;
  float v = 0.f;
  for (int g = g0; g < nblk; g += 16) v += part[g * 16 + d];
  klred[g0 * 16 + d] = v;
  __syncthreads();
  float t = 0.f;
  if (tid < 16) {
#pragma unroll
    for (int q = 0; q < 16; ++q) t += klred[q * 16 + tid];
  }
  return t;
}

__global__ __launch_bounds__(256) void k_reparam_kl_finish(const float* __restrict__ kl_part, int nblk, float* __restrict__ kl_dim,
                                                           const float* __restrict__ coef, int D) {
  __shared__ float klred[256];
  const float t = kl_blocks_sum(kl_part, nblk, klred);
  const int d = threadIdx.x;
  if (d < 16) kl_dim[d] = d < D ? t * coef[DVAE_C_INV_B] : 0.f;
}

__global__ void k_reparam_kl_bwd(const float* __restrict__ dz, const float* __restrict__ dz2,
                                 const float* __restrict__ dz3, const float* __restrict__ dmu_x,
                                 const float* __restrict__ dlv_x, const float* __restrict__ mu,
                                 const float* __restrict__ logvar, const float* __restrict__ eps,
                                 const float* __restrict__ scal, const float* __restrict__ coef,
                                 float* __restrict__ dml, int B, int D) {
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= (long)B * D) return;
  const float klw = scal[DVAE_S_KLW] * coef[DVAE_C_INV_B];
  const float m = mu[idx], lv = logvar[idx];
  float g = dz ? dz[idx] : 0.f;
  if (dz2) g += dz2[idx];                 // gradients reaching z by other routes (TC estimator, discriminator)
  if (dz3) g += dz3[idx];
  float dm, dl;
  reparam_kl_bwd_elem(klw, m, lv, g, eps, idx, &dm, &dl);
  if (dmu_x) dm += dmu_x[idx];
  if (dlv_x) dl += dlv_x[idx];
  const long b = idx / D; const int d = idx % D;
  dml[b * 2 * D + 2 * d] = dm;
  dml[b * 2 * D + 2 * d + 1] = dl;
}

// ---- reconstruction loss ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_recon_loss(const float* __restrict__ recon, const float* __restrict__ target,
                                                    long n, int dist, const float* __restrict__ coef,
                                                    float* __restrict__ partials, float* __restrict__ g,
                                                    int wrt_logit) {
  const float gs = coef[DVAE_C_INV_B];
  float acc = 0.f;
  const long n4 = n >> 2;
  const f32x4* r4 = reinterpret_cast<const f32x4*>(recon);
  const f32x4* t4 = reinterpret_cast<const f32x4*>(target);
  f32x4* g4 = reinterpret_cast<f32x4*>(g);
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n4; q += (long)gridDim.x * blockDim.x) {
    const f32x4 pv = r4[q], xv = t4[q];
    f32x4 gv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gl, gr;
      acc += recon_elem(pv[j], xv[j], dist, &gl, &gr);
      gv[j] = gs * (wrt_logit ? gl : gr);
    }
    if (g) g4[q] = gv;
  }
  __shared__ float red[4];
  float v = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = block_sum4_read(red);
}

// ---- beta-TCVAE ------------------------------------------------------------------------------
#define BTC_WG_MAX_ROWS 512      // local rows up to which the backward passes run a workgroup per row / column

// per-column constants of the Gaussian log-density, TRANSPOSED ([D][Bg]) so that the lanes of a wave
// (consecutive columns j) read 256 contiguous bytes:  muT = mu, cT = -0.5 (log 2pi + logvar),
// ivT = exp(-logvar)   (math.py:48-50)
__global__ void k_btcvae_prep(const float* __restrict__ mu, const float* __restrict__ lv, int Bg, int D,
                              float* __restrict__ tmp) {
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= (long)Bg * D) return;
  const int j = idx / D, d = idx % D;
  const float l = lv[idx];
  tmp[(long)d * Bg + j] = mu[idx];
  tmp[(long)(D + d) * Bg + j] = gauss_c(l);
  tmp[(long)(2 * D + d) * Bg + j] = expf(-l);
}

// one workgroup (4 waves) per row i: the columns j are split over the 4 waves x 64 lanes, so the
// serial online-logsumexp chain per lane is Bg/256 long (the kernel is latency-, not throughput-bound)
template <int DT>
__global__ __launch_bounds__(256) void k_btcvae_fwd(const float* __restrict__ z, const float* __restrict__ mu,
                                                    const float* __restrict__ lv, const float* __restrict__ tmp,
                                                    int Bg, int row0, int Bl, int is_mss,
                                                    const float* __restrict__ log_w, float* __restrict__ rowstats, int Drt) {
  constexpr int DM = DT ? DT : 16;          // DT = 0: latent dimension given at run time (<= 16)
  const int D = DT ? DT : Drt;
  __shared__ float red[4][2 * (DM + 1)];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int il = blockIdx.x;
  const int i = row0 + il;
  const LogW w = load_log_w(is_mss, log_w);
  const float* muT = tmp; const float* cT = tmp + (long)D * Bg; const float* ivT = tmp + (long)2 * D * Bg;
  float zi[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) zi[d] = z[(long)i * D + d];
  float mS = -INFINITY, sS = 0.f, md[DM], sd[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) { md[d] = -INFINITY; sd[d] = 0.f; }
#pragma unroll 2
  for (int j = threadIdx.x; j < Bg; j += 256) {
    const float lw = log_w_ij(i, j, Bg, w);
    float S = 0.f;
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      const float diff = zi[d] - muT[(long)d * Bg + j];
      const float ld = gauss_logdens(diff, cT[(long)d * Bg + j], ivT[(long)d * Bg + j]) + lw;
      S += ld;
      lse_push(md[d], sd[d], ld);
    }
    lse_push(mS, sS, S);
  }
  // Reduction of the (max, sum) pairs: the wave's MAX first (max butterflies, no transcendental), every lane rescales its sum
  // once, the sums are added; then the 4 waves through LDS, one thread per quantity (joint + D marginals).  (Merging (max, sum)
  // pairs stage by stage cost two exponentials and a divergent branch per pair and stage -- 66 dependent merges per wave, then
  // 33 more in ONE thread: the kernel spent most of its 30 us there.)
  auto wave_lse = [&](float& m, float& sm) {
    float M = m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    sm = wave_sum(m > -INFINITY ? sm * __expf(m - M) : 0.f);   // (a lane, or a whole wave, without columns: m = M = -inf)
    m = M;
  };
  wave_lse(mS, sS);
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) wave_lse(md[d], sd[d]);
  if (lane == 0) {
    red[wv][0] = mS; red[wv][1] = sS;
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) { red[wv][2 + 2 * d] = md[d]; red[wv][3 + 2 * d] = sd[d]; }
  }
  __shared__ float fin[DM + 1];
  __syncthreads();
  const int q = threadIdx.x;                               // quantity: 0 = joint density, 1 + d = marginal d
  if (q <= D) {
    const float M = fmaxf(fmaxf(red[0][2 * q], red[1][2 * q]), fmaxf(red[2][2 * q], red[3][2 * q]));
    const float sm = (red[0][2 * q + 1] * __expf(red[0][2 * q] - M) + red[1][2 * q + 1] * __expf(red[1][2 * q] - M)) +
                     (red[2][2 * q + 1] * __expf(red[2][2 * q] - M) + red[3][2 * q + 1] * __expf(red[3][2 * q] - M));
    fin[q] = M + logf(sm);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* rs = rowstats + (long)il * DVAE_ROWSTATS;
    float log_pz = 0.f, log_qzCx = 0.f, log_prod = 0.f;
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      const float m = mu[(long)i * D + d], l = lv[(long)i * D + d];
      const float diff = zi[d] - m;
      log_qzCx += gauss_logdens_lv(diff, l);
      log_pz += -0.5f * LOG2PI - 0.5f * (zi[d] * zi[d]);
      const float lse = fin[1 + d];
      rs[4 + d] = lse;
      log_prod += lse;
    }
    rs[0] = log_pz;
    rs[1] = fin[0];
    rs[2] = log_prod;
    rs[3] = log_qzCx;
  }
}

// row pass: dz[i] (one wave per local row i)
template <int DT>
__global__ __launch_bounds__(256) void k_btcvae_bwd_rows(const float* __restrict__ z, const float* __restrict__ mu,
                                                         const float* __restrict__ lv, const float* __restrict__ tmp,
                                                         const float* __restrict__ rowstats,
                                                         int Bg, int row0, int Bl, int is_mss,
                                                         const float* __restrict__ log_w, const float* __restrict__ coef,
                                                         float* __restrict__ dz, int Drt) {
  constexpr int DM = DT ? DT : 16;          // DT = 0: latent dimension given at run time (<= 16)
  const int D = DT ? DT : Drt;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int il = blockIdx.x * 4 + wv;
  if (il >= Bl) return;
  const int i = row0 + il;
  const LogW w = load_log_w(is_mss, log_w);
  const TcCoef k = load_tc_coef(coef, Bg);
  const float* muT = tmp; const float* cT = tmp + (long)D * Bg; const float* ivT = tmp + (long)2 * D * Bg;
  const float* rs = rowstats + (long)il * DVAE_ROWSTATS;
  const float lqz = rs[1];
  float zi[DM], lse[DM], g[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) { zi[d] = z[(long)i * D + d]; lse[d] = rs[4 + d]; g[d] = 0.f; }
#pragma unroll 2
  for (int j = lane; j < Bg; j += 64) {
    const float lw = log_w_ij(i, j, Bg, w);
    float ld[DM], r[DM];
    float S = 0.f;
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      const float iv = ivT[(long)d * Bg + j];
      const float diff = zi[d] - muT[(long)d * Bg + j];
      r[d] = diff * iv;
      ld[d] = gauss_logdens(diff, cT[(long)d * Bg + j], iv) + lw;
      S += ld[d];
    }
    const float P = __expf(S - lqz);
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      const float G = k.cP * P + k.cQ * __expf(ld[d] - lse[d]);
      g[d] -= G * r[d];
    }
  }
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) g[d] = wave_sum(g[d]);
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      // diagonal terms: alpha * log q(z_i|x_i) / B  and  -gamma' * log p(z_i) / B
      const float m = mu[(long)i * D + d], l = lv[(long)i * D + d];
      const float r = (zi[d] - m) * expf(-l);
      dz[(long)il * D + d] = g[d] - k.alpha * k.invB * r + k.gam * k.invB * zi[d];
    }
  }
}

// column pass: dmu[j], dlv[j] summed over the local rows (one wave per column j)
template <int DT>
__global__ __launch_bounds__(256) void k_btcvae_bwd_cols(const float* __restrict__ z, const float* __restrict__ mu,
                                                         const float* __restrict__ lv, const float* __restrict__ rowstats,
                                                         int Bg, int row0, int Bl, int is_mss,
                                                         const float* __restrict__ log_w, const float* __restrict__ coef,
                                                         float* __restrict__ dmu, float* __restrict__ dlv, int Drt) {
  constexpr int DM = DT ? DT : 16;          // DT = 0: latent dimension given at run time (<= 16)
  const int D = DT ? DT : Drt;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = blockIdx.x * 4 + wv;
  if (j >= Bg) return;
  const LogW w = load_log_w(is_mss, log_w);
  const TcCoef k = load_tc_coef(coef, Bg);
  float mj[DM], lj[DM], ivj[DM], gm[DM], gl[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
    mj[d] = mu[(long)j * D + d]; lj[d] = lv[(long)j * D + d]; ivj[d] = expf(-lj[d]); gm[d] = 0.f; gl[d] = 0.f;
  }
#pragma unroll 2
  for (int il = lane; il < Bl; il += 64) {
    const int i = row0 + il;
    const float* rs = rowstats + (long)il * DVAE_ROWSTATS;
    const float lw = log_w_ij(i, j, Bg, w);
    float ld[DM], r[DM], diff[DM];
    float S = 0.f;
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      diff[d] = z[(long)i * D + d] - mj[d];
      r[d] = diff[d] * ivj[d];
      const float c = gauss_c(lj[d]);
      ld[d] = gauss_logdens(diff[d], c, ivj[d]) + lw;
      S += ld[d];
    }
    const float P = __expf(S - rs[1]);
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      const float G = k.cP * P + k.cQ * __expf(ld[d] - rs[4 + d]);
      gm[d] += G * r[d];
      gl[d] += G * (-0.5f + 0.5f * r[d] * diff[d]);
    }
  }
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) { gm[d] = wave_sum(gm[d]); gl[d] = wave_sum(gl[d]); }
  if (lane == 0) {
    const bool local = (j >= row0 && j < row0 + Bl);
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      float a = gm[d], b = gl[d];
      if (local) {  // diagonal term alpha * log q(z_j|x_j) / B
        const float diff = z[(long)j * D + d] - mj[d];
        const float r = diff * ivj[d];
        a += k.alpha * k.invB * r;
        b += k.alpha * k.invB * (-0.5f + 0.5f * r * diff);
      }
      dmu[(long)j * D + d] = a;
      dlv[(long)j * D + d] = b;
    }
  }
}

// row pass with one WORKGROUP (4 waves) per local row i (round 6; up to BTC_WG_MAX_ROWS local rows): the columns j are split over
// 256 lanes, so a lane walks Bg / 256 columns instead of Bg / 64 -- the kernel is a chain of dependent L2 round trips, not
// arithmetic -- and the four waves' sums are added in a fixed order through LDS.  One rank of eight of the headline configuration
// (128 local rows x 1024 columns): 0.372 -> 0.365 ms per sharded step; 256 x 256: 0.375 -> 0.373; 1024 x 1024 level, 2048 x 2048
// 1 % slower (four times the workgroups beside the decoder's kernels): profiles/r06_s2_est1.txt.
template <int DT>
__device__ __forceinline__ void btcvae_bwd_rows_wg_body(int il, const float* __restrict__ z, const float* __restrict__ mu,
                                                        const float* __restrict__ lv, const float* __restrict__ tmp,
                                                        const float* __restrict__ rowstats,
                                                        int Bg, int row0, int Bl, int is_mss,
                                                        const float* __restrict__ log_w, const float* __restrict__ coef,
                                                        float* __restrict__ dz, int Drt) {
  constexpr int DM = DT ? DT : 16;          // DT = 0: latent dimension given at run time (<= 16)
  const int D = DT ? DT : Drt;
  __shared__ float red[4][DM];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = row0 + il;
  const LogW w = load_log_w(is_mss, log_w);
  const TcCoef k = load_tc_coef(coef, Bg);
  const float* muT = tmp; const float* cT = tmp + (long)D * Bg; const float* ivT = tmp + (long)2 * D * Bg;
  const float* rs = rowstats + (long)il * DVAE_ROWSTATS;
  const float lqz = rs[1];
  float zi[DM], lse[DM], g[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) { zi[d] = z[(long)i * D + d]; lse[d] = rs[4 + d]; g[d] = 0.f; }
#pragma unroll 2
  for (int j = threadIdx.x; j < Bg; j += 256) {
    const float lw = log_w_ij(i, j, Bg, w);
    float ld[DM], r[DM];
    float S = 0.f;
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      const float iv = ivT[(long)d * Bg + j];
      const float diff = zi[d] - muT[(long)d * Bg + j];
      r[d] = diff * iv;
      ld[d] = gauss_logdens(diff, cT[(long)d * Bg + j], iv) + lw;
      S += ld[d];
    }
    const float P = __expf(S - lqz);
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      const float G = k.cP * P + k.cQ * __expf(ld[d] - lse[d]);
      g[d] -= G * r[d];
    }
  }
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
    const float v = wave_sum(g[d]);
    if (lane == 0) red[wv][d] = v;
  }
  __syncthreads();
  const int d = threadIdx.x;
  if (d < D) {
    // diagonal terms: alpha * log q(z_i|x_i) / B  and  -gamma' * log p(z_i) / B
    const float gs = block_sum4_read(red, d);
    const float zd = z[(long)i * D + d];
    const float m = mu[(long)i * D + d], l = lv[(long)i * D + d];
    const float r = (zd - m) * expf(-l);
    dz[(long)il * D + d] = gs - k.alpha * k.invB * r + k.gam * k.invB * zd;
  }
}

// column pass with one WORKGROUP per column j (the rows are split over 256 lanes), fixed-order sum of the four waves through LDS
template <int DT>
__device__ __forceinline__ void btcvae_bwd_cols_wg_body(int j, const float* __restrict__ z, const float* __restrict__ mu,
                                                        const float* __restrict__ lv, const float* __restrict__ rowstats,
                                                        int Bg, int row0, int Bl, int is_mss,
                                                        const float* __restrict__ log_w, const float* __restrict__ coef,
                                                        float* __restrict__ dmu, float* __restrict__ dlv, int Drt) {
  constexpr int DM = DT ? DT : 16;          // DT = 0: latent dimension given at run time (<= 16)
  const int D = DT ? DT : Drt;
  __shared__ float red[4][2 * DM];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const LogW w = load_log_w(is_mss, log_w);
  const TcCoef k = load_tc_coef(coef, Bg);
  float mj[DM], lj[DM], ivj[DM], gm[DM], gl[DM];
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
    mj[d] = mu[(long)j * D + d]; lj[d] = lv[(long)j * D + d]; ivj[d] = expf(-lj[d]); gm[d] = 0.f; gl[d] = 0.f;
  }
#pragma unroll 2
  for (int il = threadIdx.x; il < Bl; il += 256) {
    const int i = row0 + il;
    const float* rs = rowstats + (long)il * DVAE_ROWSTATS;
    const float lw = log_w_ij(i, j, Bg, w);
    float ld[DM], r[DM], diff[DM];
    float S = 0.f;
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      diff[d] = z[(long)i * D + d] - mj[d];
      r[d] = diff[d] * ivj[d];
      const float c = gauss_c(lj[d]);
      ld[d] = gauss_logdens(diff[d], c, ivj[d]) + lw;
      S += ld[d];
    }
    const float P = __expf(S - rs[1]);
#pragma unroll
    for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
      const float G = k.cP * P + k.cQ * __expf(ld[d] - rs[4 + d]);
      gm[d] += G * r[d];
      gl[d] += G * (-0.5f + 0.5f * r[d] * diff[d]);
    }
  }
#pragma unroll
  for (int d = 0; d < DM; ++d) if (DT != 0 || d < D) {
    const float a = wave_sum(gm[d]), b = wave_sum(gl[d]);
    if (lane == 0) { red[wv][2 * d] = a; red[wv][2 * d + 1] = b; }
  }
  __syncthreads();
  const int d = threadIdx.x;
  if (d < D) {
    float a = block_sum4_read(red, 2 * d), b = block_sum4_read(red, 2 * d + 1);
    if (j >= row0 && j < row0 + Bl) {  // diagonal term alpha * log q(z_j|x_j) / B
      const float m = mu[(long)j * D + d], iv = expf(-lv[(long)j * D + d]);
      const float diff = z[(long)j * D + d] - m;
      const float r = diff * iv;
      a += k.alpha * k.invB * r;
      b += k.alpha * k.invB * (-0.5f + 0.5f * r * diff);
    }
    dmu[(long)j * D + d] = a;
    dlv[(long)j * D + d] = b;
  }
}

// both passes in ONE launch: workgroups [0, Bl) take a row each, [Bl, Bl + Bg) a column each (they are independent; on the
// exchange stream of a sharded step every launch is ~6 us of the chain the FC input gradients wait for)
template <int DT>
__global__ __launch_bounds__(256) void k_btcvae_bwd_wg(const float* __restrict__ z, const float* __restrict__ mu,
                                                       const float* __restrict__ lv, const float* __restrict__ tmp,
                                                       const float* __restrict__ rowstats, int Bg, int row0, int Bl, int is_mss,
                                                       const float* __restrict__ log_w, const float* __restrict__ coef,
                                                       float* __restrict__ dz, float* __restrict__ dmu, float* __restrict__ dlv, int Drt) {
  if ((int)blockIdx.x < Bl) btcvae_bwd_rows_wg_body<DT>(blockIdx.x, z, mu, lv, tmp, rowstats, Bg, row0, Bl, is_mss, log_w, coef, dz, Drt);
  else btcvae_bwd_cols_wg_body<DT>(blockIdx.x - Bl, z, mu, lv, rowstats, Bg, row0, Bl, is_mss, log_w, coef, dmu, dlv, Drt);
}

// ---- FactorVAE pieces ----------------------------------------------------------------------
__global__ void k_permute_dims(const float* __restrict__ z, const int64_t* __restrict__ perm, float* __restrict__ out,
                               int B, int D) {
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= (long)B * D) return;
  const int b = idx / D, d = idx % D;
  out[idx] = z[perm[(long)d * B + b] * D + d];
}

__global__ __launch_bounds__(256) void k_disc_losses(const float* __restrict__ lg, int Bh, const float* __restrict__ coef,
                                                     float* __restrict__ sums, float* __restrict__ g_dtc,
                                                     float* __restrict__ g_tc) {
  // single workgroup; rows [0,Bh): D(z1) target 0, rows [Bh,2Bh): D(z_perm) target 1
  float s_tc = 0.f, s_ce0 = 0.f, s_ce1 = 0.f;
  const float inv = 1.f / (float)Bh;
  const float gtc = coef[DVAE_C_ANNEAL] * coef[DVAE_C_BETA] * inv;
  for (int r = threadIdx.x; r < 2 * Bh; r += blockDim.x) {
    const float a = lg[2 * r], b = lg[2 * r + 1];
    const float mx = fmaxf(a, b);
    const float lse = mx + logf(expf(a - mx) + expf(b - mx));
    const float p0 = expf(a - lse), p1 = expf(b - lse);
    if (r < Bh) {
      s_tc += a - b;
      s_ce0 += lse - a;
      g_dtc[2 * r] = 0.5f * inv * (p0 - 1.f);
      g_dtc[2 * r + 1] = 0.5f * inv * p1;
      if (g_tc) { g_tc[2 * r] = gtc; g_tc[2 * r + 1] = -gtc; }
    } else {
      s_ce1 += lse - b;
      g_dtc[2 * r] = 0.5f * inv * p0;
      g_dtc[2 * r + 1] = 0.5f * inv * (p1 - 1.f);
    }
  }
  __shared__ float red[3][4];
  float v0 = wave_sum(s_tc), v1 = wave_sum(s_ce0), v2 = wave_sum(s_ce1);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = v0; red[1][threadIdx.x >> 6] = v1; red[2][threadIdx.x >> 6] = v2; }
  __syncthreads();
  if (threadIdx.x < 3) sums[threadIdx.x] = block_sum4_read(red[threadIdx.x]);
  if (threadIdx.x == 3) sums[3] = 0.f;
}

// ---- scalar epilogue -------------------------------------------------------------------------
// pack: local sums -> packed[DVAE_NPACK] (sum-all-reduce this buffer over ranks when sharded)
__device__ __forceinline__ void loss_pack_body(const float* __restrict__ rec_partials,
                                               const float* __restrict__ kl_dim, int D,
                                               const float* __restrict__ rowstats, int Bl,
                                               const float* __restrict__ disc_sums, float* packed,
                                               int kl_blocks, float kl_scale) {
  __shared__ float red[5][4];
  __shared__ float klred[256];
  const int tid = threadIdx.x;
  // latent dimensions above DVAE_MAX_D ("wide", include/dvae_hip.h): rowstats rows of DVAE_ROWSTATS_STRIDE(D) floats, kl_dim = D
  // FINAL values (no partial blocks), copied to packed[DVAE_WIDE_KL0 + d]; the 16 narrow KL slots stay zero
  const bool wide = D > DVAE_MAX_D;
  const int rstride = DVAE_ROWSTATS_STRIDE(D);
  // un-finished per-workgroup KL partials (dvae_reparam_kl_fwd without coef, dvae_fc_chain_fwd): same order as k_reparam_kl_finish
  const float klsum = (kl_dim && kl_blocks > 0) ? kl_blocks_sum(kl_dim + 16, kl_blocks, klred) : 0.f;
  float r = 0.f;
  for (int k = tid; k < DVAE_REC_NPART; k += 256) r += rec_partials[k];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (rowstats) {
    for (int i = tid; i < Bl; i += 256) {
      const float* rs = rowstats + (long)i * rstride;
      s0 += rs[0]; s1 += rs[1]; s2 += rs[2]; s3 += rs[3];
    }
  }
  float v[5] = {r, s0, s1, s2, s3};
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    float w = wave_sum(v[k]);
    if ((tid & 63) == 0) red[k][tid >> 6] = w;
  }
  __syncthreads();
  if (tid < 5) {
    const float t = block_sum4_read(red[tid]);
    packed[tid == 0 ? 0 : 16 + tid] = t;          // [0] rec, [17..20] rowstat sums
  }
  if (tid < 16) {
    const int d = tid;
    float v = 0.f;
    if (kl_dim && d < D && !wide) v = kl_blocks > 0 ? klsum * kl_scale : kl_dim[d];
    packed[1 + d] = v;
  }
  if (wide) {
    for (int d = tid; d < D; d += 256) packed[DVAE_WIDE_KL0 + d] = kl_dim ? kl_dim[d] : 0.f;
  }
  if (tid >= 64 && tid < 64 + 3) packed[21 + (tid - 64)] = disc_sums ? disc_sums[tid - 64] : 0.f;
  if (tid >= 96 && tid < 96 + 8) packed[24 + (tid - 96)] = 0.f;
}

__global__ __launch_bounds__(256) void k_loss_pack(const float* __restrict__ rec_partials,
                                                   const float* __restrict__ kl_dim, int D,
                                                   const float* __restrict__ rowstats, int Bl,
                                                   const float* __restrict__ disc_sums, float* __restrict__ packed) {
  loss_pack_body(rec_partials, kl_dim, D, rowstats, Bl, disc_sums, packed, 0, 0.f);
}

__device__ __forceinline__ void loss_finalize_body(int kind, const float* packed, int D, int Bg,
                                                   const float* __restrict__ coef, float* __restrict__ scal) {
  const float rec = packed[0] * coef[DVAE_C_INV_B];
  float kl = 0.f;
  const int kp = D > DVAE_MAX_D ? DVAE_WIDE_KL0 : 1, ks = D > DVAE_MAX_D ? DVAE_WIDE_KL0 : DVAE_S_KL0;   // wide layouts: dvae_hip.h
  for (int d = 0; d < D; ++d) { kl += packed[kp + d]; scal[ks + d] = packed[kp + d]; }
  const float anneal = coef[DVAE_C_ANNEAL];
  float loss = rec, klw = 0.f, mi = 0.f, tc = 0.f, dw = 0.f, dtc = 0.f;
  if (kind == DVAE_LOSS_BETAH) {
    klw = anneal * coef[DVAE_C_BETA];
    loss = rec + klw * kl;
  } else if (kind == DVAE_LOSS_BETAB) {
    const float dlt = kl - coef[DVAE_C_CAP];
    loss = rec + coef[DVAE_C_BETA] * fabsf(dlt);
    klw = coef[DVAE_C_BETA] * (dlt > 0.f ? 1.f : (dlt < 0.f ? -1.f : 0.f));
  } else if (kind == DVAE_LOSS_BTCVAE) {
    const float invB = 1.f / (float)Bg;
    const float s_pz = packed[17], s_qz = packed[18], s_prod = packed[19], s_qzcx = packed[20];
    mi = (s_qzcx - s_qz) * invB;
    tc = (s_qz - s_prod) * invB;
    dw = (s_prod - s_pz) * invB;
    loss = rec + (coef[DVAE_C_ALPHA] * mi + coef[DVAE_C_BETA] * tc + anneal * coef[DVAE_C_GAMMA] * dw);
  } else if (kind == DVAE_LOSS_FACTOR) {
    const float invh = 1.f / (float)Bg;   // Bg = (global) half batch
    tc = packed[21] * invh;
    dtc = 0.5f * (packed[22] * invh + packed[23] * invh);
    klw = 1.f;
    loss = rec + kl + anneal * coef[DVAE_C_BETA] * tc;
  }
  scal[DVAE_S_LOSS] = loss; scal[DVAE_S_REC] = rec; scal[DVAE_S_KL] = kl; scal[DVAE_S_MI] = mi;
  scal[DVAE_S_TC] = tc; scal[DVAE_S_DWKL] = dw; scal[DVAE_S_KLW] = klw; scal[DVAE_S_DTC] = dtc;
}

__global__ void k_loss_finalize(int kind, const float* __restrict__ packed, int D, int Bg,
                                const float* __restrict__ coef, float* __restrict__ scal) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  loss_finalize_body(kind, packed, D, Bg, coef, scal);
}

// single-process epilogue: pack (+ finishing the KL partials) and finalize in ONE launch
__global__ __launch_bounds__(256) void k_loss_epilogue(int kind, const float* __restrict__ rec_partials,
                                                       const float* __restrict__ kl_dim, int kl_blocks, int D,
                                                       const float* __restrict__ rowstats, int Bl,
                                                       const float* __restrict__ disc_sums, int Bg,
                                                       const float* __restrict__ coef, float* packed,
                                                       float* __restrict__ scal) {
  loss_pack_body(rec_partials, kl_dim, D, rowstats, Bl, disc_sums, packed, kl_blocks, coef[DVAE_C_INV_B]);
  if (!scal) return;
  __threadfence();
  __syncthreads();                       // packed[] was written by this workgroup
  if (threadIdx.x == 0) loss_finalize_body(kind, packed, D, Bg, coef, scal);
}

__global__ void k_sigmoid_bwd(const float* __restrict__ gy, const float* __restrict__ y, float* __restrict__ out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = gy[i] * ((1.f - y[i]) * y[i]);
}

// gradient of the per-dimension KL (losses.py:452-480: latent_kl[d] = mean_b 0.5(-1 - lv + mu^2 + e^lv)) for an arbitrary
// upstream gradient g[d]: the autograd-compatible path (loss(data, recon, latent_dist, ...) then loss.backward())
__global__ void k_kl_normal_bwd(const float* __restrict__ g, const float* __restrict__ mu, const float* __restrict__ lv,
                                float* __restrict__ dmu, float* __restrict__ dlv, int B, int D) {
  const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (idx >= (long)B * D) return;
  const float gd = g[idx % D] / (float)B;
  dmu[idx] = gd * mu[idx];
  dlv[idx] = gd * 0.5f * (expf(lv[idx]) - 1.f);
}

// dst[0] = scale * sum(src[0..n)) in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void k_reduce_sum(const float* __restrict__ src, long n, float scale, float* __restrict__ dst) {
  __shared__ float red[4];
  float a = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) a += src[i];
  const float v = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) dst[0] = scale * block_sum4_read(red);
}

// ToTensor of a uint8 image batch (utils/datasets.py:207-209): dst = float(src) / 255, 16 pixels per thread
__global__ void k_u8_to_f32(const uint8_t* __restrict__ src, float* __restrict__ dst, long n) {
  const long n16 = n >> 4;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n16; q += (long)gridDim.x * blockDim.x) {
    const uint4 v = reinterpret_cast<const uint4*>(src)[q];
    const unsigned int wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (float)((wds[k] >> (8 * j)) & 0xff) / 255.0f;
      reinterpret_cast<f32x4*>(dst)[q * 4 + k] = o;
    }
  }
  if (blockIdx.x == 0) {
    for (long i = (n16 << 4) + threadIdx.x; i < n; i += blockDim.x) dst[i] = (float)src[i] / 255.0f;
  }
}

struct Coef8 { float v[8]; };
__global__ void k_set_coef(float* __restrict__ coef, Coef8 c) {
  if (threadIdx.x < 8) coef[threadIdx.x] = c.v[threadIdx.x];
}

__global__ void k_add(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = a[i] + b[i];
}

// out = alpha * a (+ beta * b): the means over the global batch and the mirrored-world completions of the data-parallel step
__global__ void k_axpby(float* __restrict__ out, const float* __restrict__ a, float alpha, const float* __restrict__ b,
                        float beta, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = b ? alpha * a[i] + beta * b[i] : alpha * a[i];
}

// src[A][Bn][inner] -> dst[Bn][A][inner]: the packed exchanges of the sharded beta-TCVAE step (an all-gather delivers
// [world][3][B*D], the estimator reads [3][world*B*D]; its column gradients [2][world][B*D] leave as [world][2][B*D])
__global__ void k_swap_outer(const float* __restrict__ src, float* __restrict__ dst, int A, int Bn, int inner) {
  // one workgroup per (a, b) slab: no per-element index division
  const int a = blockIdx.x / Bn, b = blockIdx.x % Bn;
  const float* s = src + (long)blockIdx.x * inner;
  float* d = dst + ((long)b * A + a) * inner;
  if ((inner & 3) == 0 && (((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
    for (int i = threadIdx.x; i < inner / 4; i += blockDim.x)
      reinterpret_cast<f32x4*>(d)[i] = reinterpret_cast<const f32x4*>(s)[i];
  } else {
    for (int i = threadIdx.x; i < inner; i += blockDim.x) d[i] = s[i];
  }
}

// ---- launchers -------------------------------------------------------------------------------
int launch_reparam_kl_fwd(const float* ml, const float* eps, float* mu, float* logvar, float* z, float* kl_dim,
                          const float* coef, int B, int D, hipStream_t s) {
  if (D > DVAE_MAX_D) return launch_reparam_kl_fwd_wide(ml, eps, mu, logvar, z, kl_dim, coef, B, D, s);
  // kl_dim[16..16+RK_BLOCKS*16) is used as scratch for the per-workgroup partial sums
  const int blocks = reparam_kl_blocks(B);
  float* part = kl_dim ? kl_dim + 16 : nullptr;
  hipLaunchKernelGGL(k_reparam_kl_fwd, dim3(blocks), dim3(256), 0, s, ml, eps, mu, logvar, z, part, B, D);
  DVAE_CHECK_LAUNCH();
  if (kl_dim && coef) {      // coef == NULL: the raw partials stay in kl_dim[16..]; dvae_loss_epilogue finishes them
    hipLaunchKernelGGL(k_reparam_kl_finish, dim3(1), dim3(256), 0, s, part, blocks, kl_dim, coef, D);
    DVAE_CHECK_LAUNCH();
  }
  return 0;
}

int launch_reparam_kl_bwd(const float* dz, const float* dz2, const float* dz3, const float* dmu_x, const float* dlv_x,
                          const float* mu, const float* logvar,
                          const float* eps, const float* scal, const float* coef, float* dml, int B, int D,
                          hipStream_t s) {
  long n = (long)B * D;
  hipLaunchKernelGGL(k_reparam_kl_bwd, dim3((n + 255) / 256), dim3(256), 0, s, dz, dz2, dz3, dmu_x, dlv_x, mu, logvar, eps,
                     scal, coef, dml, B, D);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_recon_loss(const float* recon, const float* target, long n, int dist, const float* coef, float* partials,
                      float* g, int wrt_logit, hipStream_t s) {
  hipLaunchKernelGGL(k_recon_loss, dim3(DVAE_REC_NPART), dim3(256), 0, s, recon, target, n, dist, coef, partials, g,
                     wrt_logit);
  DVAE_CHECK_LAUNCH();
  return 0;
}

// latent_dim 10 (every reference experiment) has fully unrolled kernels <10>; any other D <= DVAE_MAX_D runs the same code
// <0> with the dimension as a run-time bound (the kernels' last argument)
#define BTC_LAUNCH_D(kern, grid, ...)                                                         \
  do {                                                                                        \
    if (D == 10) hipLaunchKernelGGL(kern<10>, grid, dim3(256), 0, s, __VA_ARGS__, D);         \
    else hipLaunchKernelGGL(kern<0>, grid, dim3(256), 0, s, __VA_ARGS__, D);                  \
    DVAE_CHECK_LAUNCH();                                                                      \
  } while (0)

int launch_btcvae_fwd(const float* z, const float* mu, const float* lv, int Bg, int D, int row0, int Bl, int is_mss,
                      const float* log_w, float* tmp, float* rowstats, hipStream_t s) {
  if (D < 1) return 1;
  const long n = (long)Bg * D;
  hipLaunchKernelGGL(k_btcvae_prep, dim3((n + 255) / 256), dim3(256), 0, s, mu, lv, Bg, D, tmp);
  DVAE_CHECK_LAUNCH();
  if (D > DVAE_MAX_D) return launch_btcvae_fwd_wide(z, mu, lv, Bg, D, row0, Bl, is_mss, log_w, tmp, rowstats, s);   // latent_wide.hip
  BTC_LAUNCH_D(k_btcvae_fwd, dim3(Bl), z, mu, lv, tmp, Bg, row0, Bl, is_mss, log_w, rowstats);
  return 0;
}

int launch_btcvae_bwd(const float* z, const float* mu, const float* lv, const float* rowstats, int Bg, int D, int row0,
                      int Bl, int is_mss, const float* log_w, const float* coef, const float* tmp, float* dz, float* dmu,
                      float* dlv, hipStream_t s) {
  if (D < 1) return 1;
  if (D > DVAE_MAX_D)
    return launch_btcvae_bwd_wide(z, mu, lv, rowstats, Bg, D, row0, Bl, is_mss, log_w, coef, tmp, dz, dmu, dlv, s);
  // a workgroup per row / column up to BTC_WG_MAX_ROWS local rows (both passes in one launch), a wave per row / column above:
  // see k_btcvae_bwd_wg
  if (Bl <= BTC_WG_MAX_ROWS) {
    BTC_LAUNCH_D(k_btcvae_bwd_wg, dim3(Bl + Bg), z, mu, lv, tmp, rowstats, Bg, row0, Bl, is_mss, log_w, coef, dz, dmu, dlv);
    return 0;
  }
  BTC_LAUNCH_D(k_btcvae_bwd_rows, dim3((Bl + 3) / 4), z, mu, lv, tmp, rowstats, Bg, row0, Bl, is_mss, log_w, coef, dz);
  BTC_LAUNCH_D(k_btcvae_bwd_cols, dim3((Bg + 3) / 4), z, mu, lv, rowstats, Bg, row0, Bl, is_mss, log_w, coef, dmu, dlv);
  return 0;
}

int launch_permute_dims(const float* z, const int64_t* perm, float* out, int B, int D, hipStream_t s) {
  long n = (long)B * D;
  hipLaunchKernelGGL(k_permute_dims, dim3((n + 255) / 256), dim3(256), 0, s, z, perm, out, B, D);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_disc_losses(const float* lg, int Bh, const float* coef, float* sums, float* g_dtc, float* g_tc,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_disc_losses, dim3(1), dim3(256), 0, s, lg, Bh, coef, sums, g_dtc, g_tc);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_loss_pack(const float* rec_partials, const float* kl_dim, int D, const float* rowstats, int Bl,
                     const float* disc_sums, float* packed, hipStream_t s) {
  hipLaunchKernelGGL(k_loss_pack, dim3(1), dim3(256), 0, s, rec_partials, kl_dim, D, rowstats, Bl, disc_sums, packed);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int reparam_kl_blocks(int B) {            // the grid of launch_reparam_kl_fwd = the number of partial blocks it leaves
  int blocks = (B + 255) / 256;
  return blocks > RK_BLOCKS ? RK_BLOCKS : blocks;
}

int launch_kl_finish(float* kl_dim, int kl_blocks, const float* coef, int D, hipStream_t s) {
  hipLaunchKernelGGL(k_reparam_kl_finish, dim3(1), dim3(256), 0, s, kl_dim + 16, kl_blocks, kl_dim, coef, D);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_loss_epilogue(int kind, const float* rec_partials, const float* kl_dim, int kl_blocks, int D, const float* rowstats,
                         int Bl, const float* disc_sums, int Bg, const float* coef, float* packed, float* scal,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_loss_epilogue, dim3(1), dim3(256), 0, s, kind, rec_partials, kl_dim, kl_blocks, D, rowstats, Bl,
                     disc_sums, Bg, coef, packed, scal);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_loss_finalize(int kind, const float* packed, int D, int Bg, const float* coef, float* scal, hipStream_t s) {
  hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(64), 0, s, kind, packed, D, Bg, coef, scal);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_sigmoid_bwd(const float* gy, const float* y, float* out, long n, hipStream_t s) {
  long g = (n + 255) / 256; if (g > 4096) g = 4096;
  hipLaunchKernelGGL(k_sigmoid_bwd, dim3(g), dim3(256), 0, s, gy, y, out, n);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_kl_normal_bwd(const float* g, const float* mu, const float* lv, float* dmu, float* dlv, int B, int D, hipStream_t s) {
  const long n = (long)B * D;
  hipLaunchKernelGGL(k_kl_normal_bwd, dim3((n + 255) / 256), dim3(256), 0, s, g, mu, lv, dmu, dlv, B, D);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_reduce_sum(const float* src, long n, float scale, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_sum, dim3(1), dim3(256), 0, s, src, n, scale, dst);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_u8_to_f32(const uint8_t* src, float* dst, long n, hipStream_t s) {
  long g = ((n >> 4) + 255) / 256; if (g > 4096) g = 4096; if (g < 1) g = 1;
  hipLaunchKernelGGL(k_u8_to_f32, dim3(g), dim3(256), 0, s, src, dst, n);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_set_coef(float* coef, const float* v, hipStream_t s) {
  Coef8 c;
  for (int i = 0; i < 8; ++i) c.v[i] = v[i];
  hipLaunchKernelGGL(k_set_coef, dim3(1), dim3(64), 0, s, coef, c);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_add(const float* a, const float* b, float* out, long n, hipStream_t s) {
  long g = (n + 255) / 256; if (g > 2048) g = 2048;
  hipLaunchKernelGGL(k_add, dim3(g), dim3(256), 0, s, a, b, out, n);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_axpby(float* out, const float* a, float alpha, const float* b, float beta, long n, hipStream_t s) {
  long g = (n + 255) / 256; if (g > 2048) g = 2048;
  hipLaunchKernelGGL(k_axpby, dim3(g), dim3(256), 0, s, out, a, alpha, b, beta, n);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int launch_swap_outer(const float* src, float* dst, int A, int Bn, long inner, hipStream_t s) {
  hipLaunchKernelGGL(k_swap_outer, dim3(A * Bn), dim3(256), 0, s, src, dst, A, Bn, (int)inner);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // namespace dvae
