// Latent-space arithmetic shared by the estimator kernels: the training losses (loss.hip, latent_wide.hip, fc_chain.hip), the
// entropy estimator (metrics.hip), the per-image scores (loglik.hip) and the ELBO decomposition (elbo_decomp.hip).  The ONE
// definition in csrc/ of log 2 pi, the stratified-sampling weight, the beta-TCVAE coefficient set, the Gaussian log-density / KL /
// reparameterisation-backward elements, the online-logsumexp steps and the fixed-order four-wave reductions.  These kernels
// are compared against one oracle and against each other ("the same arithmetic with a run-time D"): the operation order of
// every helper is part of its contract, and a change here is gated on the machine code of its callers (tools/isa_identity.py).
// Included at the end of common.h.
#pragma once

namespace dvae {

#define LOG2PI 1.8378770664093453f

// ---- stratified-sampling weights and beta-TCVAE coefficients ------------------------------------------------------------
// log of the three distinct entries of the importance-weight matrix (math.py:53-73): 1/N, the stratified weight, 1/M; all
// zero when minibatch stratified sampling is off (minibatch weighted sampling puts its constant elsewhere: losses.py:535-544)
struct LogW { float lN, lS, lM; };
__device__ __forceinline__ LogW load_log_w(int is_mss, const float* __restrict__ log_w) {
  return {is_mss ? log_w[0] : 0.f, is_mss ? log_w[1] : 0.f, is_mss ? log_w[2] : 0.f};
}
__device__ __forceinline__ float log_w_ij(int i, int j, int Bg, const LogW& w) {
  // math.py:66-72 with M+1 == B: column 0 <- 1/N, column 1 <- strat, then W[M-1,0] <- strat
  const float lN = w.lN, lS = w.lS, lM = w.lM;      // values first: a ?: between members selects an ADDRESS, and the struct
  if (j == 0) return (i == Bg - 2) ? lS : lN;       // then lives in (LDS-promoted) memory instead of registers
  if (j == 1) return lS;
  return lM;
}

// weights of the estimator's gradient (losses.py:523-544): gam = gamma * anneal; cP multiplies the joint softmax term
// exp(S_ij - log q(z_i)), cQ the marginal ones exp(ld_ijd - lse_id); alpha and gam weigh the diagonal terms
struct TcCoef { float alpha, beta, gam, invB, cP, cQ; };
__device__ __forceinline__ TcCoef load_tc_coef(const float* __restrict__ coef, int Bg) {
  TcCoef k;
  k.alpha = coef[DVAE_C_ALPHA]; k.beta = coef[DVAE_C_BETA]; k.gam = coef[DVAE_C_GAMMA] * coef[DVAE_C_ANNEAL];
  k.invB = 1.f / (float)Bg;
  k.cP = (k.beta - k.alpha) * k.invB; k.cQ = (k.gam - k.beta) * k.invB;
  return k;
}

// ---- elements ---------------------------------------------------------------------------------------------------------------
// log_density_gaussian (math.py:48-50) from the per-column constants c = -0.5 (log 2pi + logvar), iv = exp(-logvar) and
// diff = z - mu
__device__ __forceinline__ float gauss_c(float lv) { return -0.5f * (LOG2PI + lv); }
__device__ __forceinline__ float gauss_logdens(float diff, float c, float iv) { return c - 0.5f * (diff * diff * iv); }
// the same from the log-variance itself (the diagonal terms log q(z_i | x_i))
__device__ __forceinline__ float gauss_logdens_lv(float diff, float lv) { return gauss_c(lv) - 0.5f * (diff * diff * expf(-lv)); }

// KL(N(m, e^lv) || N(0, 1)) of one latent element (losses.py:470)
__device__ __forceinline__ float kl_elem(float m, float lv) { return 0.5f * (-1.f - lv + m * m + expf(lv)); }

// gradient of  z = m + exp(lv / 2) eps  (vae.py:66-68; eps == NULL: z = m) and of klw * kl_elem(m, lv) for an upstream
// gradient g of z: *dm, *dl.  `o` = the element's index in eps.
__device__ __forceinline__ void reparam_kl_bwd_elem(float klw, float m, float lv, float g, const float* __restrict__ eps, long o,
                                                    float* dm, float* dl) {
  *dm = g + klw * m;
  *dl = klw * 0.5f * (expf(lv) - 1.f);
  if (eps) *dl += g * eps[o] * 0.5f * expf(0.5f * lv);
}

// ---- online logsumexp: running (max m, sum s of exp(v - m)) --------------------------------------------------------------
// branch-free push: the wave never diverges; __expf = v_exp_f32(x*log2e).  For FINITE v only: (-inf, 0) + -inf is NaN.
__device__ __forceinline__ void lse_push(float& m, float& s, float v) {
  const float mn = fmaxf(m, v);
  s = s * __expf(m - mn) + __expf(v - mn);
  m = mn;
}
// eight values per rescale (9 v_exp_f32 per 8 densities), and values that can be -inf (exp(-logvar) overflowing, a padding
// record): while everything so far is -inf the shift is 0, so that exp(-inf - shift) = 0 instead of exp(-inf + inf) = NaN;
// torch.logsumexp returns -inf for such a column too.  (k_entropy_lse of metrics.hip keeps this step and its one-value
// form for the tail written out: see there.)
__device__ __forceinline__ void lse_fold8(const float (&v)[8], float& m, float& s) {
  float mx = m;
#pragma unroll
  for (int u = 0; u < 8; ++u) mx = fmaxf(mx, v[u]);
  const float sh = mx > -INFINITY ? mx : 0.f;
  float t = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) t += __expf(v[u] - sh);
  s = s * __expf(m - sh) + t;
  m = mx;
}
// merge of another partial (m2, s2) into (m, s): updates s, RETURNS the new m (`m = lse_merge(m, s, m2, s2)`; with both
// by reference the compiler ordered the callers' registers differently).  An empty partial (-inf, 0) leaves (m, s) alone.
__device__ __forceinline__ float lse_merge(float m, float& s, float m2, float s2) {
  if (m2 > m) { s = s * __expf(m - m2) + s2; m = m2; }
  else if (m2 > -INFINITY) { s += s2 * __expf(m2 - m); }
  return m;
}

// ---- fixed-order reductions over the 4 waves of a 256-thread workgroup, through LDS -------------------------------------
// Two forms.  For a result that thread 0 (or threads < k, one quantity each) consumes, the call site keeps its own producer
// side -- wave_sum, lane 0 of wave w stores to red[w] (or red[w][q], quantity q of N), ONE barrier for all quantities -- and
// the consumers call block_sum4_read.  (A helper for the producer side changed the machine code of every caller.)  For a
// result that every thread needs: block_sum4 / block_max4, which carry both barriers (the leading one: `red` may still be
// read from a previous use).
__device__ __forceinline__ float block_sum4_read(const float (&red)[4]) { return (red[0] + red[1]) + (red[2] + red[3]); }
template <int N>
__device__ __forceinline__ float block_sum4_read(const float (&red)[4][N], int q) {
  return (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
}
__device__ __forceinline__ float block_sum4(float v, float (&red)[4]) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return block_sum4_read(red);
}
__device__ __forceinline__ float block_max4(float v, float (&red)[4]) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

}  // namespace dvae
