/*
 * libdvae_unsup_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the label-free scores of
 * Evaluator.compute_unsupervised_scores (disentanglement_lib's unsupervised_metrics: Gaussian total correlation, Gaussian
 * Wasserstein correlation, mean pairwise mutual information of the discretised latents): one pass over the table of posterior
 * means for the full D x D covariance, and one for the D (D - 1) / 2 joint histograms of every pair of discretised latents.  A
 * sixth library next to libdvae_hip.so (include/dvae_hip.h), libdvae_eval_hip.so (include/dvae_eval_hip.h),
 * libdvae_score_hip.so (include/dvae_score_hip.h), libdvae_info_hip.so (include/dvae_info_hip.h) and libdvae_irs_hip.so
 * (include/dvae_irs_hip.h): nothing here is part of the training step and nothing here is recorded into a launch plan.  The
 * reference (YannDubs/disentangling-vae) has no counterpart.
 *
 * Conventions, as in dvae_info_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (fp64 / int64 / int32 where stated), aligned to its element size and no more;
 *     sizes are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation);
 *     workspace is caller-provided and needs no initialisation;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_unsup_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - every floating-point reduction has a fixed order (no float atomics) and the counters are integers: the same inputs
 *     give the same bits.
 *
 * table: fp32 [N, D], one ROW per data point (the posterior means), 1 <= D <= DVAE_UNSUP_MAX_D.  The data set needs no factors
 * of variation: nothing here knows of lat_sizes.
 * rows: int64 [S] row numbers, every entry in [0, N) -- the CALLER checks that, the device does not -- repeats allowed; or
 * NULL: all N rows in order (S is then ignored and taken as N).  N and S are at most 2^31 - 1, so no count overflows int32.
 */
#ifndef DVAE_UNSUP_HIP_H
#define DVAE_UNSUP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_UNSUP_VERSION 1

/* limits: D above DVAE_UNSUP_MAX_D and n_bins above DVAE_UNSUP_MAX_BINS are refused (a bin is kept in a byte, a row of the
 * table in one staged line)                                                                                                  */
#define DVAE_UNSUP_MAX_D 64
#define DVAE_UNSUP_MAX_BINS 64
/* Both passes cut the S selected rows into equal chunks, one workgroup per chunk (and, for the histograms, per tile of pairs):
 * ceil(S / BLOCK_ROWS) of them, at most DVAE_UNSUP_MAX_BLOCKS -- from there on the chunks grow instead.                      */
#define DVAE_UNSUP_MOMENTS_BLOCK_ROWS 1024
#define DVAE_UNSUP_HIST_BLOCK_ROWS 4096
#define DVAE_UNSUP_MAX_BLOCKS 1024
/* the moments pass keeps D (D + 3) / 2 sums -- D of x_d and D (D + 1) / 2 of x_d x_e, d <= e -- one per thread, the 256 threads
 * of a workgroup taking up to this many each (ceil(MAX_D (MAX_D + 3) / 2 / 256)); the second one starts at D = 22.           */
#define DVAE_UNSUP_MOMENTS_THREAD_SUMS 9
/* a workgroup of the histogram pass counts a tile of consecutive pairs in LDS: as many pairs as this many int32 counters hold,
 * n_bins^2 each, and one pair at least (20 bins: 10 pairs; 64 bins: 1).  16 KB of counters, 37 KB with the staged bins and
 * edges: four workgroups share a CU's 160 KB.                                                                                 */
#define DVAE_UNSUP_HIST_LDS_INTS 4096

int dvae_unsup_version(void);
const char* dvae_unsup_last_error(void);

/* ---- moments of the selected rows ------------------------------------------------------------------------------------------
 * x_s = table[rows[s], :], s < S:
 *   col_min[d], col_max[d]   fp32 [D]: the smallest / largest x_sd, the fp32 elements themselves
 *   col_mean[d]              fp64 [D]: the mean of x_.d
 *   cov[d, e]                fp64 [D, D]: the unbiased (ddof = 1) covariance of x_.d and x_.e; both triangles are written from
 *                            one value (bitwise symmetric); all zeros when S = 1
 * The sums are taken of x - x_0 (the first selected row), each element converted to fp64 BEFORE the subtraction:
 * sum (x_d - x0_d) and sum (x_d - x0_d)(x_e - x0_e) in fp64 registers, the rows of a chunk in order, the chunks combined in a
 * fixed order; never E[xy] - E[x] E[y] of the raw values.
 * col_mean and cov are fp64 and are NEVER rounded to fp32: the Gaussian total correlation takes the log-determinant of cov, and
 * a covariance rounded to fp32 costs cond(cov) x 6e-8 of it -- whole digits for the near-singular matrices of a trained model.
 * ws: dvae_unsup_moments_ws_floats(N, D, S) floats (S <= 0: as for NULL rows; 0 for other sizes out of range).               */
size_t dvae_unsup_moments_ws_floats(long N, int D, long S);
int dvae_unsup_moments(const float* table, const int64_t* rows, long N, int D, long S, float* ws, float* col_min,
                       float* col_max, double* col_mean, double* cov, void* stream);

/* ---- joint histograms of every pair of latents ----------------------------------------------------------------------------
 * edges fp32 [D, n_bins]: the lower edge of every bin of latent d, ascending.  bin_d(x) = #{j : edges[d,j] <= x} - 1, clamped to
 * [0, n_bins) (numpy.digitize(x, edges[d]) - 1): comparisons only, no arithmetic on x -- the rule of dvae_info_joint_hist.
 * counts int32 [P, n_bins, n_bins], P = D (D - 1) / 2: pair p = (d, e), d < e, in lexicographic order ((0,1), (0,2), ...,
 * (0,D-1), (1,2), ...),
 *   counts[p, b, c] = #{s : bin_d(x_sd) = b and bin_e(x_se) = c};
 * every element is written, whatever counts and ws held before.  D = 1 has no pair and is an invalid argument.
 * ws: dvae_unsup_pair_hist_ws_floats(...) floats (currently 0 always: ws may be NULL).                                       */
size_t dvae_unsup_pair_hist_ws_floats(long N, int D, long S, int n_bins);
int dvae_unsup_pair_hist(const float* table, const int64_t* rows, const float* edges, long N, int D, long S, int n_bins,
                         float* ws, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
