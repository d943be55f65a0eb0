/*
 * libdvae_mmd_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the InfoVAE / MMD-VAE training loss (Zhao, Song & Ermon
 * 2019; the MMD regulariser of WAE-MMD, Tolstikhin et al. 2018): the unbiased maximum mean discrepancy between a batch of
 * latent samples z [B, D] and as many prior samples p [B, D], and its gradient with respect to z.  A tenth library next to
 * libdvae_hip.so (include/dvae_hip.h), the seven score libraries and libdvae_dip_hip.so; nothing of it is linked into another.
 * Like libdvae_dip_hip.so it IS part of the training step: InfoVaeLoss (disvae_amd/models/losses.py) issues its two launches
 * behind the step's loss epilogue and hands the gradients to dvae_fc_chain_bwd / dvae_reparam_kl_bwd as dmu_x / dlv_x.  The
 * reference (YannDubs/disentangling-vae) has no counterpart.
 *
 * For z, p fp32 [B, D], r^2(a, b) = sum_d (a_d - b_d)^2 and bandwidth h > 0:
 *   rbf:  k(a, b) = exp(-r^2 / h)                               d_a k = -(2 / h) k (a - b)
 *   imq:  k(a, b) = sum_s C_s / (C_s + r^2),  C_s = h s,        d_a k = -2 sum_s C_s / (C_s + r^2)^2 (a - b)
 *         s in {0.1, 0.2, 0.5, 1, 2, 5, 10}   (WAE's sum of inverse multiquadrics)
 *   S_zz = sum_{i != j} k(z_i, z_j),  S_pp = sum_{i != j} k(p_i, p_j),  S_zp = sum_{i, j} k(z_i, p_j)
 *   MMD_u = (S_zz + S_pp) / (B (B - 1)) - 2 S_zp / B^2          (the U-statistic; B = 1: MMD_u = 0 with zero gradients)
 *   dMMD_u/dz_i = 2 / (B (B - 1)) sum_{j != i} d_a k(z_i, z_j) - 2 / B^2 sum_j d_a k(z_i, p_j)
 *   dmu = w dMMD_u/dz,   dlv = w dMMD_u/dz * (z - mu) / 2       (z = mu + eps exp(logvar / 2): no eps is needed)
 * r^2 is ALWAYS the sum of the squared differences (every float converted to fp64 first, so a_d - b_d is exact), never
 * |a|^2 + |b|^2 - 2 a.b, which cancels when the samples sit far from the origin or close to one another.
 *
 * Conventions:
 *   - z, p, mu, dmu, dlv, loss_io are DEVICE pointers to fp32, aligned to 4 bytes and no more; ws and out are DEVICE pointers
 *     to fp64, aligned to 8 bytes and no more; sizes are element counts;
 *   - 1 <= D <= DVAE_MMD_MAX_D, 1 <= B <= DVAE_MMD_MAX_B, kernel one of DVAE_MMD_RBF / DVAE_MMD_IMQ, h finite and > 0, w
 *     finite; anything else returns <0 (text via dvae_mmd_last_error(), per thread) before any launch;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work: no allocation, no synchronisation, no copy;
 *     the workspace is caller-provided and needs no initialisation;
 *   - r^2 is fp64; the kernel function and its derivative are evaluated in fp32 on the rounded r^2; the three value sums and
 *     every gradient sum are fp64 and have a fixed order; there are no float atomics, no cooperative launch, and no workgroup
 *     waits on another (the launch boundary between the two entry points is the only ordering): the same inputs give the same
 *     bits.
 */
#ifndef DVAE_MMD_HIP_H
#define DVAE_MMD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_MMD_VERSION 1

/* D above DVAE_MMD_MAX_D and B above DVAE_MMD_MAX_B are refused                                                               */
#define DVAE_MMD_MAX_D 128
#define DVAE_MMD_MAX_B 65536
/* the `kernel` argument                                                                                                       */
#define DVAE_MMD_RBF 0
#define DVAE_MMD_IMQ 1
/* a workgroup                                                                                                                 */
#define DVAE_MMD_THREADS 256
/* The pair launch tiles the rows (the B rows of z, then the B rows of p) by DVAE_MMD_ROWS: 2 ceil(B / DVAE_MMD_ROWS) row tiles.
 * A z tile meets all 2 B columns (z, then p), a p tile the B columns of p.  The columns of a tile are cut into equal chunks,
 * one per workgroup: ceil(columns / DVAE_MMD_COLS) of them, at most DVAE_MMD_MAX_CGROUPS -- from there on the chunks grow
 * instead, and a workgroup walks its chunk in trips of DVAE_MMD_COLS columns (the first B with a second trip:
 * DVAE_MMD_COLS * DVAE_MMD_MAX_CGROUPS / 2 + 1 for a z tile, DVAE_MMD_COLS * DVAE_MMD_MAX_CGROUPS + 1 for a p tile).            */
#define DVAE_MMD_ROWS 16
#define DVAE_MMD_COLS 32
#define DVAE_MMD_MAX_CGROUPS 8

int dvae_mmd_version(void);
const char* dvae_mmd_last_error(void);

/* doubles of workspace for a [B, D] batch: 4 ceil(B / ROWS) G value records of two doubles + B G D gradient partials, G the
 * column chunks of a z tile; 0 for sizes out of range                                                                         */
size_t dvae_mmd_ws_doubles(long B, int D);

/* ---- pair sums --------------------------------------------------------------------------------------------------------------
 * Workgroup (row tile, column chunk) adds k over its pairs in fp64 -- a z tile into (S_zz, S_zp), a p tile into S_pp, pairs
 * i == j of the same table left out by INDEX -- and, with with_grad != 0, a z tile adds for each of its rows the D sums
 * sum_j c_ij (z_id - x_jd), c_ij = 2 / (B (B - 1)) k' (z columns, j != i) or -2 / B^2 k' (p columns), over the columns of its
 * chunk in order.  One value record per workgroup and one gradient partial per (row, chunk) go to ws.                          */
int dvae_mmd_pairs(const float* z, const float* p, long B, int D, int kernel, double h, int with_grad, double* ws, void* stream);

/* ---- value and gradients ------------------------------------------------------------------------------------------------------
 * ws: what dvae_mmd_pairs left for the SAME z, p, B, D, kernel, h (with_grad != 0 when dmu is given).  The records are added in
 * the order of the tiles and chunks.
 *   out      fp64 [5]: w MMD_u, MMD_u, S_zz, S_pp, S_zp; every element is written
 *   dmu      fp32 [B, D] = w dMMD_u/dz, or NULL: the value only (evaluation); every element is written
 *   dlv      fp32 [B, D] = w dMMD_u/dz * (z - mu) / 2, or NULL; needs mu and dmu; every element is written
 *   loss_io  fp32 [1] or NULL: *loss_io += (float)(w MMD_u), by one thread -- the step's scalar loss becomes the total
 * The gradients are those of w MMD_u itself: a caller whose loss is a batch mean adds them unscaled (as dvae_dip_grad's).       */
int dvae_mmd_finish(const float* z, const float* mu, long B, int D, double w, const double* ws, float* dmu, float* dlv,
                    double* out, float* loss_io, void* stream);

#ifdef __cplusplus
}
#endif
#endif
