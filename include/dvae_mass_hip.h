/*
 * libdvae_mass_hip.so -- C-ABI of the MI355X (gfx950) kernels behind Evaluator.compute_interpretability_scores: the factor-based
 * scores of Do & Tran 2020 ("Theory and Evaluation Metrics for Learning Disentangled Representations"), RMIG and JEMMIG, and the
 * two scores the same mutual-information matrix gives, MIG-sup (Li et al. 2020) and DCIMIG (Sepliarskaia et al. 2019).  What is
 * computed here is the POSTERIOR MASS table: q(z_d | x) of every selected row integrated over fixed bins and summed per value of
 * every factor of variation.  A twelfth library next to libdvae_hip.so (include/dvae_hip.h): nothing here is part of the training
 * step and nothing here is recorded into a launch plan.  The reference (YannDubs/disentangling-vae) has no counterpart.
 *
 * Conventions, as in dvae_info_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (fp64 / int64 / int32 where stated), aligned to its element size and no more;
 *     sizes are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation);
 *     workspace is caller-provided and needs no initialisation;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_mass_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - no atomics, no cooperative launch, no workgroup waits on another: every sum has a fixed order, the same inputs give the
 *     same bits.
 *
 * mean, logvar: fp32 [N, D], one ROW per data point (q(z|x) in data-set order), any D >= 1.  The data set enumerates
 * lat_sizes [K] (int32, every entry >= 1) in row-major order: factor k of table row r takes the value
 * v_k(r) = (r / stride_k) % lat_sizes[k], stride_k = prod(lat_sizes[k+1:]).  No factor value is ever stored.
 * rows: int64 [S] row numbers, every entry in [0, N) -- the CALLER checks that, the device does not -- repeats allowed; or
 * NULL: all N rows in order (S is then ignored and taken as N).
 */
#ifndef DVAE_MASS_HIP_H
#define DVAE_MASS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_MASS_VERSION 1

/* limits: K above DVAE_MASS_MAX_FACTORS and n_bins above DVAE_MASS_MAX_BINS are refused                                    */
#define DVAE_MASS_MAX_FACTORS 8
#define DVAE_MASS_MAX_BINS 256
/* A wave holds DVAE_MASS_WAVE_BINS + 1 consecutive bin edges, one per lane, and owns the DVAE_MASS_WAVE_BINS bins between them
 * (the last edge of a wave is the first of the next, evaluated twice): a workgroup is ceil(n_bins / DVAE_MASS_WAVE_BINS) waves. */
#define DVAE_MASS_WAVE_BINS 63
/* The S selected rows are cut into equal chunks, one workgroup per (chunk, latent, column group): ceil(S / BLOCK_ROWS) chunks,
 * at most DVAE_MASS_MAX_CHUNKS -- from there on the chunks grow instead.  A workgroup walks its chunk in trips of
 * DVAE_MASS_TRIP_ROWS rows.                                                                                                  */
#define DVAE_MASS_BLOCK_ROWS 256
#define DVAE_MASS_MAX_CHUNKS 128
#define DVAE_MASS_TRIP_ROWS 64
/* A workgroup keeps its accumulators in LDS, at most this many doubles: n_bins for each of floor(LDS_DOUBLES / n_bins) COLUMNS,
 * a column being one value of one factor (sum_sizes of them).  More columns than that are split evenly over
 * ceil(sum_sizes / that many) column groups (gridDim.z), each of which walks the rows again -- so no lat_sizes is refused.      */
#define DVAE_MASS_LDS_DOUBLES 20000

int dvae_mass_version(void);
const char* dvae_mass_last_error(void);

/* ---- posterior mass per bin and factor value -------------------------------------------------------------------------------
 * edges fp64 [n_bins - 1], ascending: e_1 .. e_{n_bins-1}; bin 0 is (-inf, e_1), bin b is [e_b, e_{b+1}), bin n_bins - 1 is
 * [e_{n_bins-1}, +inf) (n_bins = 1: edges is not read and may be NULL).  For row r and latent d, in fp64 from the fp32 inputs:
 *   sigma = exp(logvar[r,d] / 2),  t_j = (e_j - mean[r,d]) / (sigma sqrt(2)),  up_j = erfc(t_j) / 2,  dn_j = erfc(-t_j) / 2
 *   Q_0 = dn_1,  Q_{n_bins-1} = up_{n_bins-1},  Q_b = up_b - up_{b+1} if t_b >= 0 else dn_{b+1} - dn_b      (n_bins = 1: Q_0 = 1)
 * ALWAYS the difference of the two smaller tails, never Phi(b) - Phi(a) with Phi = (1 + erf) / 2.  The tail on the far side of
 * the mean, which the rule needs only next to the mean and in the two end bins, is formed as 1 - (the near tail).
 * mass fp64: for latent d and factor k the block [n_bins, lat_sizes[k]],
 *   mass[d * n_bins * sum_sizes + n_bins * sum(lat_sizes[:k]) + b * lat_sizes[k] + v] = sum_{s : v_k(rows[s]) = v} Q_b(rows[s], d)
 * (d-major, then k: the layout of dvae_info_joint_hist's counts), summed in the order of s within a chunk and then over the
 * chunks in their order; every element is written, whatever mass and ws held before.  sum_sizes = sum(lat_sizes), which the
 * caller knows; the device checks it against lat_sizes (a mismatch leaves every element 0).  D * n_bins * sum_sizes <= 2^31 - 1,
 * D <= 16384.
 * ws: dvae_mass_ws_doubles(N, D, K, S, n_bins, sum_sizes) doubles (S <= 0: as for NULL rows; 0 for sizes out of range).        */
size_t dvae_mass_ws_doubles(long N, int D, int K, long S, int n_bins, long sum_sizes);
int dvae_mass_joint(const float* mean, const float* logvar, const int64_t* rows, const int32_t* lat_sizes, const double* edges,
                    long N, int D, int K, long S, int n_bins, long sum_sizes, double* ws, double* mass, void* stream);

#ifdef __cplusplus
}
#endif
#endif
