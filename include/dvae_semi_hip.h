/*
 * libdvae_semi_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the semi-supervised training loss S2-beta-VAE (Locatello et
 * al. 2020, "Disentangling Factors of Variation Using Few Labels"; disentanglement_lib's semi_supervised_vae.py): the supervised
 * regulariser R_sup that ties latent k to factor k on the labelled rows of a batch, and its gradient with respect to the
 * posterior means.  A seventeenth library next to libdvae_hip.so (include/dvae_hip.h), the score libraries and the three other
 * loss plugins; nothing of it is linked into another.  It IS part of the training step: SemiSupervisedVaeLoss
 * (disvae_amd/models/losses.py) issues its two launches behind the step's loss epilogue and hands the gradient to
 * dvae_fc_chain_bwd / dvae_reparam_kl_bwd as dmu_x.  The reference (YannDubs/disentangling-vae) has no counterpart.
 *
 * Labels never exist in memory.  The data set enumerates its factors of variation by row number, rows[i] is the row number of
 * image i of the batch (NEGATIVE: the image is unlabelled) and the value of factor k of a labelled image is
 *   v_ik = (rows[i] / strides[k]) % sizes[k]                                      k < K <= D: factor k is tied to latent k.
 * With L the labelled rows, n_lab = |L|, mu fp32 [n, D] and y_ik = v_ik / sizes[k]:
 *   DVAE_SEMI_XENT  R = sum_{i in L} sum_{k<K} max(x, 0) - x y_ik + log1p(exp(-|x|)),  x = mu_ik;   dR/dmu_ik = sigmoid(mu_ik) - y_ik
 *   DVAE_SEMI_L2    R = sum_{i in L} sum_{k<K} (mu_ik - y_ik)^2;                                     dR/dmu_ik = 2 (mu_ik - y_ik)
 *   DVAE_SEMI_COV   R = sum_{d<D, k<K, d != k} C_dk^2,  C_dk = 1/n_lab sum_{i in L} (mu_id - m_d)(v_ik - vbar_k)  (m, vbar: means
 *                   over L; the value INDICES, not normalised);                  dR/dmu_id = (2 / n_lab) sum_{k != d} C_dk (v_ik - vbar_k)
 * DVAE_SEMI_MEAN divides R and the gradient of XENT and L2 by n_lab (COV is what it is under both reductions).  n_lab = 0:
 * R = 0, C = 0 and every gradient is 0.
 *
 * Conventions:
 *   - mu, dmu, w, loss_io are DEVICE pointers to fp32, aligned to 4 bytes and no more; rows is a DEVICE pointer to int64, ws and
 *     out DEVICE pointers to fp64, aligned to 8 bytes and no more; sizes and strides are HOST pointers to K int64 each, read
 *     during the call (their values travel as kernel arguments); sizes are element counts;
 *   - mu_interleaved = 0: mu is [n, D], element (i, d) at i D + d; 1: mu is the mean half of the interleaved [n, 2 D] output of
 *     mu_logvar_gen, element (i, d) at 2 i D + 2 d;
 *   - 1 <= n <= DVAE_SEMI_MAX_ROWS, 1 <= K <= DVAE_SEMI_MAX_K, K <= D <= DVAE_SEMI_MAX_D, sizes[k] >= 1, strides[k] >= 1;
 *     anything else returns <0 (text via dvae_semi_last_error(), per thread) before any launch;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work: no allocation, no synchronisation, no copy; the
 *     workspace is caller-provided and needs no initialisation;
 *   - every sum is fp64 and has a fixed order; there are no atomics, no cooperative launch, and no workgroup waits on another
 *     (the launch boundary between the two entry points is the only ordering): the same inputs give the same bits.
 */
#ifndef DVAE_SEMI_HIP_H
#define DVAE_SEMI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_SEMI_VERSION 1

/* D, K, n above these are refused                                                                                             */
#define DVAE_SEMI_MAX_D 64
#define DVAE_SEMI_MAX_K 8
#define DVAE_SEMI_MAX_ROWS 16384
/* a workgroup                                                                                                                 */
#define DVAE_SEMI_THREADS 256
/* The rows are cut into chunks of DVAE_SEMI_BLOCK_ROWS, one per workgroup (of both launches): ceil(n / DVAE_SEMI_BLOCK_ROWS)
 * of them, 256 at most.                                                                                                       */
#define DVAE_SEMI_BLOCK_ROWS 64
/* the `kind` argument                                                                                                         */
#define DVAE_SEMI_XENT 0
#define DVAE_SEMI_L2 1
#define DVAE_SEMI_COV 2
/* the `reduction` argument                                                                                                    */
#define DVAE_SEMI_SUM 0
#define DVAE_SEMI_MEAN 1

int dvae_semi_version(void);
const char* dvae_semi_last_error(void);

/* doubles of workspace for n rows: ceil(n / DVAE_SEMI_BLOCK_ROWS) * (2 + D + K + D K), for every kind; 0 for sizes out of
 * range                                                                                                                       */
size_t dvae_semi_ws_doubles(long n, int D, int K);

/* ---- partial sums ---------------------------------------------------------------------------------------------------------------
 * Every workgroup adds, over the labelled rows of its chunk in order, one record of 2 + D + K + D K doubles into ws:
 *   [0] the number of labelled rows, [1] the chunk's part of R (XENT, L2; COV: 0) and, for COV only (else not written),
 *   [2, 2 + D) sum (mu_id - mu_0d), [2 + D, 2 + D + K) sum (v_ik - v_0k), then sum (mu_id - mu_0d)(v_ik - v_0k) at d K + k,
 * where row 0 is the FIRST labelled row of the batch (every float converted to fp64 first, so the differences are exact).     */
int dvae_semi_partials(const float* mu, int mu_interleaved, const int64_t* rows, long n, int D, int K, const int64_t* sizes,
                       const int64_t* strides, int kind, double* ws, void* stream);

/* ---- value and gradient ---------------------------------------------------------------------------------------------------------
 * ws: what dvae_semi_partials left for the SAME mu, rows, n, D, K, sizes, strides, kind.  Every workgroup adds the records in
 * the order of the chunks, so every workgroup holds the same bits of n_lab, C and G = dR/dC.
 *   w        fp32 [1] on the DEVICE: the weight of the term, read by the kernel (a launch that is replayed sees the value of
 *            the moment it runs)
 *   out      fp64 [2 + D K]: R (after `reduction`, NOT multiplied by w), n_lab, then C [D, K] row-major (XENT, L2: zeros); every
 *            element is written
 *   dmu      fp32 [n, D] = w dR/dmu, or NULL: the value only (evaluation); every element is written -- exact zeros on
 *            unlabelled rows and, for XENT and L2, on columns >= K
 *   loss_io  fp32 [1] or NULL: *loss_io += (float)(w R), by one thread -- the step's scalar loss becomes the total
 * The gradient is that of w R itself: a caller whose loss is a batch mean adds it unscaled.                                   */
int dvae_semi_grad(const float* mu, int mu_interleaved, const int64_t* rows, long n, int D, int K, const int64_t* sizes,
                   const int64_t* strides, int kind, int reduction, const float* w, const double* ws, float* dmu, double* out,
                   float* loss_io, void* stream);

#ifdef __cplusplus
}
#endif
#endif
