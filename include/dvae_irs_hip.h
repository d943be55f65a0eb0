/*
 * libdvae_irs_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the interventional robustness score (Suter et al. 2019;
 * disentanglement_lib's irs.py) of Evaluator.compute_irs: the mean of every latent over every group of rows that share a
 * (binned) factor value, and exact order statistics -- an exact segmented selection -- of the absolute deviations from a given
 * centre per group.  A fifth library next to libdvae_hip.so (include/dvae_hip.h), libdvae_eval_hip.so (include/dvae_eval_hip.h),
 * libdvae_score_hip.so (include/dvae_score_hip.h) and libdvae_info_hip.so (include/dvae_info_hip.h): nothing here is part of
 * the training step and nothing here is recorded into a launch plan.  The reference (YannDubs/disentangling-vae) has no
 * counterpart.
 *
 * Conventions, as in dvae_info_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (int64 / int32 where stated), aligned to its element size and no more; sizes
 *     are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation, no host round
 *     trip); workspace is caller-provided and needs no initialisation;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_irs_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - every floating-point reduction has a fixed order (no float atomics) and every atomic is an integer add, min or max: the
 *     same inputs give the same bits.
 *
 * table: fp32 [N, D], one ROW per data point (the posterior means in data-set order), D >= 1.  The data set enumerates
 * lat_sizes [K] (int32, every entry >= 1) in row-major order: factor k of table row r takes the value
 * v_k(r) = (r / stride_k) % lat_sizes[k], stride_k = prod(lat_sizes[k+1:]).  No factor value is ever stored.
 * rows: int64 [S] row numbers, every entry in [0, N) -- the CALLER checks that, the device does not -- repeats allowed; or
 * NULL: all N rows in order (S is then ignored and taken as N).  S <= 2^31 - 1.
 *
 * Groups.  group_of_value int32 [sum_sizes], sum_sizes = sum(lat_sizes): entry sum(lat_sizes[:k]) + v is the group, in
 * [0, n_groups[k]), of value v of factor k (an entry outside that range leaves the value's rows out of every group of factor k).
 * n_groups int32 [K], every entry in [1, max_groups].  The group index space: slot 0 is "all selected rows"; the groups of
 * factor k start at 1 + sum(n_groups[:k]); total_groups = 1 + sum(n_groups).  sum_sizes, total_groups and max_groups (>= every
 * n_groups[k]) are what the CALLER knows of the device arrays; the device checks them against lat_sizes / n_groups, and a
 * mismatch writes zeros to every output element and touches nothing else.
 */
#ifndef DVAE_IRS_HIP_H
#define DVAE_IRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_IRS_VERSION 1

/* limits: K above DVAE_IRS_MAX_FACTORS and max_groups above DVAE_IRS_MAX_GROUPS are refused */
#define DVAE_IRS_MAX_FACTORS 8
#define DVAE_IRS_MAX_GROUPS 256
/* launch shapes.  The means pass walks a row in pieces of DVAE_IRS_MEANS_COLS floats.  Both entries cut the S selected rows into
 * equal chunks, one workgroup per chunk (and per factor; the selection also per latent): ceil(S / BLOCK_ROWS) of them, at most
 * DVAE_IRS_MAX_BLOCKS -- from there on the chunks grow instead.                                                              */
#define DVAE_IRS_MEANS_COLS 16
#define DVAE_IRS_MEANS_BLOCK_ROWS 1024
#define DVAE_IRS_SELECT_BLOCK_ROWS 4096
#define DVAE_IRS_MAX_BLOCKS 512
/* a selection workgroup keeps the 256-bin digit histograms of at most this many groups of one factor in LDS; a factor with more
 * groups is served by several workgroups per chunk, each taking a slice of that many groups (there is no global-memory path)  */
#define DVAE_IRS_SELECT_LDS_GROUPS 40
/* the selection is a radix select on the bit patterns of the non-negative fp32 deviations: this many passes of 8 bits, then one
 * pass for the next larger element and the largest: a fixed number of passes whatever the data                               */
#define DVAE_IRS_SELECT_PASSES 4

int dvae_irs_version(void);
const char* dvae_irs_last_error(void);

/* ---- counts and means of every group ---------------------------------------------------------------------------------------
 * x_s = table[rows[s], :], s < S.  counts int32 [total_groups]: the number of selected rows in the group.  means fp32
 * [total_groups, D]: the mean of x_.d over the group's rows -- fp64 sums of x - x_0 (x_0 the first selected row) in a fixed order,
 * x_0 + sum / count rounded to fp32 once; a column that is constant over the selection has exactly that constant as every mean.
 * An empty group gets count 0 and mean 0.  Every element is written, whatever the outputs and ws held before.
 * ws: dvae_irs_group_means_ws_floats(...) floats (S <= 0: as for NULL rows; 0 for sizes the entry refuses): one record of
 * (2 D + 1) total_groups words per chunk.                                                                                    */
size_t dvae_irs_group_means_ws_floats(long N, int D, int K, long S, int total_groups);
int dvae_irs_group_means(const float* table, const int64_t* rows, const int32_t* lat_sizes, const int32_t* group_of_value,
                         const int32_t* n_groups, long N, int D, int K, long S, long sum_sizes, int total_groups, int max_groups,
                         float* ws, int32_t* counts, float* means, void* stream);

/* ---- order statistics of the absolute deviations of every group ------------------------------------------------------------
 * centres fp32 [total_groups, D] and rank int32 [total_groups] are INPUTS.  dev_sd = |x_sd - centres[g, d]| (one fp32
 * subtraction, one absolute value) for the rows s of group g; n_g of them.  stat_lo, stat_hi, dev_max fp32 [total_groups, D]:
 * the rank[g]-th smallest dev (0-based), the (rank[g] + 1)-th smallest (equal to stat_lo when rank[g] = n_g - 1) and the largest
 * -- elements of the multiset of deviations, bit for bit.  A rank outside [0, n_g) (-1: "skip this group"; any rank of an
 * empty group) writes +0 to all three for that group.  total_groups * D <= DVAE_IRS_MAX_PAIRS.
 * ws: dvae_irs_group_order_stats_ws_floats(...) floats: 256 + 5 words per (group, latent) pair.                               */
#define DVAE_IRS_MAX_PAIRS 4194304
size_t dvae_irs_group_order_stats_ws_floats(long N, int D, int K, long S, int total_groups);
int dvae_irs_group_order_stats(const float* table, const int64_t* rows, const int32_t* lat_sizes, const int32_t* group_of_value,
                               const int32_t* n_groups, const float* centres, const int32_t* rank, long N, int D, int K, long S,
                               long sum_sizes, int total_groups, int max_groups, float* ws, float* stat_lo, float* stat_hi,
                               float* dev_max, void* stream);

#ifdef __cplusplus
}
#endif
#endif
