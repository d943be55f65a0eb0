/*
 * libdvae_dip_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the DIP-VAE-I / DIP-VAE-II training losses (Kumar et al.
 * 2018; disentanglement_lib's DIPVAE): the biased covariance of a batch of posterior means, the regulariser that pulls it
 * towards the identity, and the regulariser's gradients with respect to the means and the log-variances.  A ninth library next
 * to libdvae_hip.so (include/dvae_hip.h) and the seven score libraries; nothing of it is linked into another.  It IS part of the
 * training step: DipVaeLoss (disvae_amd/models/losses.py) issues its two launches behind the step's loss epilogue and hands the
 * gradients to dvae_fc_chain_bwd / dvae_reparam_kl_bwd as dmu_x / dlv_x.  The reference (YannDubs/disentangling-vae) has no
 * counterpart.
 *
 * For mu, logvar fp32 [B, D], m = mean_b mu_b:
 *   Cov_mu = 1/B sum_b (mu_b - m)(mu_b - m)^T
 *   C      = Cov_mu                                    logvar == NULL  (DIP-VAE-I)
 *   C      = Cov_mu + diag(1/B sum_b exp(logvar_b))    logvar given    (DIP-VAE-II)
 *   R_od   = lambda_od sum_{d != e} C_de^2,  R_d = lambda_d sum_d (C_dd - 1)^2,  R = R_od + R_d
 *   G      = dR/dC:  G_de = 2 lambda_od C_de (d != e),  G_dd = 2 lambda_d (C_dd - 1)
 *   dR/dmu_b = (2 / B) G (mu_b - m),   dR/dlogvar_bd = G_dd exp(logvar_bd) / B   (DIP-VAE-II)
 *
 * Conventions:
 *   - mu, logvar, dmu, dlv, loss_io are DEVICE pointers to fp32, aligned to 4 bytes and no more; ws and out are DEVICE pointers
 *     to fp64, aligned to 8 bytes and no more; sizes are element counts;
 *   - 1 <= D <= DVAE_DIP_MAX_D, 1 <= B <= 2^31 - 1; anything else returns <0 (text via dvae_dip_last_error(), per thread) before
 *     any launch;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work: no allocation, no synchronisation, no copy;
 *     the workspace is caller-provided and needs no initialisation;
 *   - every sum is fp64 and has a fixed order; there are no float atomics, no cooperative launch, and no workgroup waits on
 *     another (the launch boundary between the two entry points is the only ordering): the same inputs give the same bits.
 */
#ifndef DVAE_DIP_HIP_H
#define DVAE_DIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_DIP_VERSION 1

/* D above DVAE_DIP_MAX_D is refused                                                                                           */
#define DVAE_DIP_MAX_D 128
/* a workgroup                                                                                                                 */
#define DVAE_DIP_THREADS 256
/* The rows are cut into equal chunks, one per workgroup (of both launches): ceil(B / DVAE_DIP_BLOCK_ROWS) of them, at most
 * DVAE_DIP_MAX_GROUPS -- from there on the chunks grow instead, and a workgroup walks its chunk in trips of
 * DVAE_DIP_BLOCK_ROWS rows (the first B with a second trip: DVAE_DIP_BLOCK_ROWS * DVAE_DIP_MAX_GROUPS + 1).                 */
#define DVAE_DIP_BLOCK_ROWS 32
#define DVAE_DIP_MAX_GROUPS 64

int dvae_dip_version(void);
const char* dvae_dip_last_error(void);

/* doubles of workspace for a [B, D] batch: groups * (2 D + D D); 0 for sizes out of range                                     */
size_t dvae_dip_ws_doubles(long B, int D);

/* ---- partial moments ------------------------------------------------------------------------------------------------------------
 * Every workgroup adds, over the rows of its chunk in order and around the shift x0 = mu[0, :] (every float converted to fp64
 * first, so x - x0 is exact), sum (x - x0)_d, sum (x - x0)_d (x - x0)_e for d <= e and, with logvar, sum exp(logvar)_d, and
 * stores one record per chunk into ws.  logvar may be NULL (DIP-VAE-I).                                                       */
int dvae_dip_moments(const float* mu, const float* logvar, long B, int D, double* ws, void* stream);

/* ---- value and gradients --------------------------------------------------------------------------------------------------------
 * ws: what dvae_dip_moments left for the SAME mu, logvar (NULL or not), B, D.  Every workgroup adds the records in the order of
 * the chunks, so every workgroup holds the same bits of C and G.
 *   out      fp64 [3 + D D]: R, R_od, R_d, then C row-major (bitwise symmetric); every element is written
 *   dmu      fp32 [B, D] = dR/dmu, or NULL: the value only (evaluation); every element is written
 *   dlv      fp32 [B, D] = dR/dlogvar, or NULL; needs logvar and dmu; every element is written
 *   loss_io  fp32 [1] or NULL: *loss_io += (float)R, by one thread -- the step's scalar loss becomes the total
 * The gradients are those of R itself: a caller whose loss is a batch mean adds them unscaled.                                */
int dvae_dip_grad(const float* mu, const float* logvar, long B, int D, double lambda_od, double lambda_d, const double* ws,
                  float* dmu, float* dlv, double* out, float* loss_io, void* stream);

#ifdef __cplusplus
}
#endif
#endif
