/*
 * libdvae_info_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the discretised MIG (Locatello et al. 2019), the
 * modularity score (Ridgeway & Mozer 2018) and the continuous-factor SAP score (Kumar et al. 2018) of
 * Evaluator.compute_information_scores: one pass over the table of posterior means for the centred moments of every
 * (latent, factor) pair, and one for the D x K family of joint histograms.  A fourth library next to libdvae_hip.so
 * (include/dvae_hip.h), libdvae_eval_hip.so (include/dvae_eval_hip.h) and libdvae_score_hip.so (include/dvae_score_hip.h):
 * nothing here is part of the training step and nothing here is recorded into a launch plan.  The reference
 * (YannDubs/disentangling-vae) has no counterpart.
 *
 * Conventions, as in dvae_score_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (int64 / int32 where stated), aligned to its element size and no more; sizes
 *     are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation);
 *     workspace is caller-provided and needs no initialisation;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_info_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - every floating-point reduction has a fixed order (no float atomics) and the counters are integers: the same inputs
 *     give the same bits.
 *
 * table: fp32 [N, D], one ROW per data point (the posterior means in data-set order), any D >= 1.  The data set enumerates
 * lat_sizes [K] (int32, every entry >= 1) in row-major order: factor k of table row r takes the value
 * v_k(r) = (r / stride_k) % lat_sizes[k], stride_k = prod(lat_sizes[k+1:]).  No factor value is ever stored.
 * rows: int64 [S] row numbers, every entry in [0, N) -- the CALLER checks that, the device does not -- repeats allowed; or
 * NULL: all N rows in order (S is then ignored and taken as N).
 */
#ifndef DVAE_INFO_HIP_H
#define DVAE_INFO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_INFO_VERSION 1

/* limits: K above DVAE_INFO_MAX_FACTORS and n_bins above DVAE_INFO_MAX_BINS are refused (a wave holds one bin per lane) */
#define DVAE_INFO_MAX_FACTORS 8
#define DVAE_INFO_MAX_BINS 64
/* launch shapes.  The moments pass gives a row the lanes of its D floats padded to one of these widths (D <= NARROW, <= MID,
 * else WAVE; a row of more than DVAE_INFO_ROW_LANES_WAVE floats is walked in pieces of that many).                          */
#define DVAE_INFO_ROW_LANES_NARROW 4
#define DVAE_INFO_ROW_LANES_MID 16
#define DVAE_INFO_ROW_LANES_WAVE 64
/* Both passes cut the S selected rows into equal chunks, one workgroup per chunk (and, for the histograms, per latent):
 * ceil(S / BLOCK_ROWS) of them, at most DVAE_INFO_MAX_BLOCKS -- from there on the chunks grow instead.                     */
#define DVAE_INFO_MOMENTS_BLOCK_ROWS 1024
#define DVAE_INFO_HIST_BLOCK_ROWS 4096
#define DVAE_INFO_MAX_BLOCKS 1024
/* one latent's n_bins * sum(lat_sizes) counters are kept in LDS by every workgroup and added to `counts` at its end when
 * they number at most this many; above, every add goes to `counts` in global memory directly.                              */
#define DVAE_INFO_HIST_LDS_INTS 8192

int dvae_info_version(void);
const char* dvae_info_last_error(void);

/* ---- moments of the selected rows ------------------------------------------------------------------------------------------
 * x_s = table[rows[s], :], v_s = the factor values of TABLE ROW rows[s] as floats, s < S:
 *   col_min[d], col_max[d]   the smallest / largest x_sd: the fp32 elements themselves
 *   col_mean[d], col_var[d]  mean and unbiased (ddof = 1) variance of x_.d
 *   cov_zv[d,k]              unbiased covariance of x_.d and v_.k
 *   factor_mean[k], factor_var[k]
 * Variances and covariances are 0 when S = 1.  The sums are taken of x - x_0 and v - v_0 (the first selected row) in fp64, and
 * never as E[x^2] - E[x]^2 of the raw values; the results are rounded to fp32 once.
 * ws: dvae_info_moments_ws_floats(N, D, K, S) floats (S <= 0: as for NULL rows; 0 for other non-positive sizes).           */
size_t dvae_info_moments_ws_floats(long N, int D, int K, long S);
int dvae_info_moments(const float* table, const int64_t* rows, const int32_t* lat_sizes, long N, int D, int K, long S,
                      float* ws, float* col_min, float* col_max, float* col_mean, float* col_var, float* cov_zv,
                      float* factor_mean, float* factor_var, void* stream);

/* ---- joint histograms of every (latent, factor) pair -----------------------------------------------------------------------
 * edges fp32 [D, n_bins]: the lower edge of every bin of latent d, ascending.  bin_d(x) = #{j : edges[d,j] <= x} - 1, clamped to
 * [0, n_bins) (numpy.digitize(x, edges[d]) - 1): comparisons only, no arithmetic on x.
 * counts int32: for latent d and factor k the block [n_bins, lat_sizes[k]],
 *   counts[d * n_bins * sum_sizes + n_bins * sum(lat_sizes[:k]) + b * lat_sizes[k] + v] = #{s : bin_d(x_sd) = b and v_sk = v}
 * (d-major, then k); every element is written, whatever counts and ws held before.  sum_sizes = sum(lat_sizes), which the
 * caller knows; the device checks it against lat_sizes (a mismatch leaves every count 0).  D * n_bins * sum_sizes <= 2^31 - 1.
 * ws: dvae_info_hist_ws_floats(...) floats (currently 0 always: ws may be NULL).                                            */
size_t dvae_info_hist_ws_floats(long N, int D, int K, long S, int n_bins, long sum_sizes);
int dvae_info_joint_hist(const float* table, const int64_t* rows, const int32_t* lat_sizes, const float* edges, long N, int D,
                         int K, long S, int n_bins, long sum_sizes, float* ws, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
