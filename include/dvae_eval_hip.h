/*
 * libdvae_eval_hip.so -- C-ABI of the evaluation-side MI355X (gfx950) kernels: the data-set level ELBO decomposition of
 * Chen et al. 2018 (beta-TCVAE, section 3) behind Evaluator.compute_elbo_decomposition.  A second library next to
 * libdvae_hip.so (include/dvae_hip.h): nothing here is part of the training step and nothing here is recorded into a
 * launch plan.  The reference (YannDubs/disentangling-vae) has no counterpart.
 *
 * Conventions, as in dvae_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (int64 where stated), aligned to its element size and no more; sizes are
 *     element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation);
 *     workspace is caller-provided and needs no initialisation;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_eval_last_error(), per thread);
 *   - no atomics: every reduction has a fixed order, the same inputs give the same bits.
 */
#ifndef DVAE_EVAL_HIP_H
#define DVAE_EVAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_EVAL_VERSION 1

/* Data points per workgroup of the joint log-density kernel: a data set of at most DVAE_EVAL_JOINT_CHUNK points is one
 * chunk, a larger one is cut into up to DVAE_EVAL_JOINT_MAX_CHUNKS chunks of at least this many points (fewer chunks when
 * the samples alone fill the device) whose partial (max, sum) pairs are merged in chunk order.                          */
#define DVAE_EVAL_JOINT_CHUNK 2048
#define DVAE_EVAL_JOINT_MAX_CHUNKS 256

int dvae_eval_version(void);
const char* dvae_eval_last_error(void);

/* ---- joint log-density under the aggregate posterior --------------------------------------------------------------------
 * logqz[s] = logsumexp_{n<N} sum_{d<D} log N(z[s,d]; mean[n,d], exp(logvar[n,d])) - log N,   s < S
 * H_joint[0] = -1/S sum_s logqz[s]  (fixed order)
 * z[S,D]: the samples, one ROW per sample; mean, logvar [N,D]: q(z|x) of the whole data set.  A sample without any finite
 * density gives logqz = -inf (never NaN).  ws: dvae_eval_joint_logq_ws_floats(N, D, S) floats (0 for non-positive sizes;
 * non-decreasing in N and in S).                                                                                         */
size_t dvae_eval_joint_logq_ws_floats(long N, int D, long S);
int dvae_eval_joint_logq(const float* z, const float* mean, const float* logvar, long N, int D, long S, float* ws,
                         float* logqz, float* H_joint, void* stream);

/* ---- per-sample terms that need only the sample's own row ---------------------------------------------------------------
 * logqz_condx[s] = sum_d [ -0.5 (log 2pi + logvar[rows[s],d]) - 0.5 eps[s,d]^2 ]     (log q(z_s | x_n(s)), z = mu + sigma eps)
 * logpz[s]       = sum_d [ -0.5 log 2pi - 0.5 z[s,d]^2 ]                             (log p(z_s), p = N(0, I))
 * means[0] = 1/S sum_s logqz_condx[s], means[1] = 1/S sum_s logpz[s]  (fixed order)
 * z, eps [S,D]; logvar [N,D]; rows: int64 [S], every entry in [0, N) -- the CALLER checks that, the device does not.       */
int dvae_eval_sample_terms(const float* z, const float* eps, const float* logvar, const int64_t* rows, long N, int D, long S,
                           float* logqz_condx, float* logpz, float* means, void* stream);

#ifdef __cplusplus
}
#endif
#endif
