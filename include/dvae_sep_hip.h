/*
 * libdvae_sep_hip.so -- C-ABI of the MI355X (gfx950) kernels behind Evaluator.compute_separability_scores: the SEPIN / WSEPIN
 * separability and informativeness scores of Do & Tran 2020 ("Theory and Evaluation Metrics for Learning Disentangled
 * Representations").  Every score is a combination of entropies under the aggregate posterior q(z) = 1/N sum_n q(z|x_n);
 * what is computed here is the LEAVE-ONE-OUT joint log-density of every latent dimension, the joint one beside it, and the
 * conditional entropy per dimension.  An eleventh library next to libdvae_hip.so (include/dvae_hip.h): nothing here is part of
 * the training step and nothing here is recorded into a launch plan.  The reference (YannDubs/disentangling-vae) has no
 * counterpart.
 *
 * Conventions, as in dvae_eval_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (fp64 / int64 where stated), aligned to its element size and no more; sizes
 *     are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation);
 *     workspace is caller-provided and needs no initialisation;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_sep_last_error(), per thread), before any launch;
 *   - no atomics, no cooperative launch, no workgroup waits on another: every reduction has a fixed order, the same inputs
 *     give the same bits.
 */
#ifndef DVAE_SEP_HIP_H
#define DVAE_SEP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_SEP_VERSION 1

/* Largest number of latent dimensions: D above it is refused.                                                           */
#define DVAE_SEP_MAX_D 64
/* D up to DVAE_SEP_TEMPLATE_D runs a kernel compiled for its width (D rounded up to an even number) that keeps all D + 1
 * logsumexp states of a sample in registers; above it a run-time-D kernel keeps DVAE_SEP_GROUP of the D + 1 states per
 * workgroup and the groups are spread over gridDim.z.                                                                   */
#define DVAE_SEP_TEMPLATE_D 16
#define DVAE_SEP_GROUP 16
/* Data points per workgroup: a data set of at most DVAE_SEP_CHUNK points is one chunk, a larger one is cut into up to
 * DVAE_SEP_MAX_CHUNKS chunks of at least this many points (fewer chunks when the samples alone fill the device) whose
 * partial (max, sum) pairs are merged in chunk order.                                                                   */
#define DVAE_SEP_CHUNK 2048
#define DVAE_SEP_MAX_CHUNKS 256

int dvae_sep_version(void);
const char* dvae_sep_last_error(void);

/* ---- leave-one-out and joint log-densities under the aggregate posterior -----------------------------------------------
 * With t_d(s, n) = log N(z[s,d]; mean[n,d], exp(logvar[n,d])):
 *   logq[i, s] = logsumexp_{n<N} sum_{d != i} t_d(s, n) - log N,   i < D      (log q_{!=i}(z_s); D = 1: the empty sum, 0)
 *   logq[D, s] = logsumexp_{n<N} sum_{d < D}  t_d(s, n) - log N               (log q(z_s), from the same pass)
 *   H[i] = -1/S sum_s logq[i, s],   i <= D   (fp64, fixed order)
 * The sum over d != i is formed by ADDING the other terms, never as the whole sum minus t_i.
 * z[S,D]: the samples, one ROW per sample; mean, logvar [N,D]: q(z|x) of the whole data set; logq: fp32 [D + 1, S];
 * H: fp64 [D + 1].  A sample without any finite density gives -inf (never NaN).  1 <= D <= DVAE_SEP_MAX_D.
 * ws: dvae_sep_loo_logq_ws_floats(N, D, S) floats (0 for sizes out of range; non-decreasing in N and in S).               */
size_t dvae_sep_loo_logq_ws_floats(long N, int D, long S);
int dvae_sep_loo_logq(const float* z, const float* mean, const float* logvar, long N, int D, long S, float* ws, float* logq,
                      double* H, void* stream);

/* ---- conditional entropy per dimension ---------------------------------------------------------------------------------
 * H_cond_d[i] = 1/S sum_s 0.5 (log 2pi + logvar[rows[s], i] + eps[s, i]^2),   i < D      (fp64, fixed order)
 *             = -1/S sum_s log q(z_si | x_n(s))  for z = mu + sigma eps.
 * eps [S,D]; logvar [N,D]; rows: int64 [S], every entry in [0, N) -- the CALLER checks that, the device does not;
 * H_cond_d: fp64 [D].  1 <= D <= DVAE_SEP_MAX_D.                                                                         */
int dvae_sep_cond_terms(const float* eps, const float* logvar, const int64_t* rows, long N, int D, long S, double* H_cond_d,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
