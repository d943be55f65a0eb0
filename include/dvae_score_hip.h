/*
 * libdvae_score_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the FactorVAE score (Kim & Mnih 2018, section 4) and
 * the beta-VAE score (Higgins et al. 2017, section 3) of Evaluator.compute_factor_scores: statistics of tens of thousands of
 * groups of rows gathered from the table of posterior means, and the majority vote on top of them.  A third library next to
 * libdvae_hip.so (include/dvae_hip.h) and libdvae_eval_hip.so (include/dvae_eval_hip.h): nothing here is part of the training
 * step and nothing here is recorded into a launch plan.  The reference (YannDubs/disentangling-vae) has no counterpart.
 *
 * Conventions, as in dvae_eval_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (int64 / int32 where stated), aligned to its element size and no more; sizes
 *     are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation);
 *     workspace is caller-provided and needs no initialisation;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_score_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - every floating-point reduction has a fixed order (no float atomics): the same inputs give the same bits.
 *
 * table: fp32 [N, D], one ROW per data point (the posterior means in data-set order).  rows: int64 row numbers, every entry
 * in [0, N) -- the CALLER checks that, the device does not.  D is a run-time value, any D >= 1.
 */
#ifndef DVAE_SCORE_HIP_H
#define DVAE_SCORE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_SCORE_VERSION 1

/* Launch shapes of the two group statistics: a group of at most DVAE_SCORE_WAVE_MAX_L rows is reduced by ONE wave (four
 * groups per workgroup, wave-level reductions only); a longer one by a whole workgroup that loops over its rows.          */
#define DVAE_SCORE_WAVE_MAX_L 256
/* dvae_score_vote counts in LDS (integer adds, one workgroup) when the K * D counters number at most this many, else with
 * one thread per counter that walks the V groups in order.                                                               */
#define DVAE_SCORE_VOTE_LDS_BINS 8192

int dvae_score_version(void);
const char* dvae_score_last_error(void);

/* ---- unbiased variance of every group ------------------------------------------------------------------------------------
 * out[v,d] = 1/(L-1) sum_{l<L} (x_l - m)^2 [* inv_scale[d]],  x_l = table[rows[v,l], d],  m = 1/L sum_l x_l,   v < V, d < D
 * computed around the group's mean (never as E[x^2] - E[x]^2).  rows [V,L], L >= 2; inv_scale [D] or NULL.
 * ws: dvae_score_group_var_ws_floats(N, D, V, L) floats (0 for non-positive sizes; currently 0 always: ws may be NULL).   */
size_t dvae_score_group_var_ws_floats(long N, int D, long V, long L);
int dvae_score_group_var(const float* table, const int64_t* rows, long N, int D, long V, long L, const float* inv_scale,
                         float* ws, float* out, void* stream);

/* ---- mean absolute difference of every group of pairs --------------------------------------------------------------------
 * out[v,d] = 1/L sum_{l<L} | table[rows_a[v,l], d] - table[rows_b[v,l], d] |,   rows_a, rows_b [V,L], L >= 1               */
int dvae_score_pair_absdiff(const float* table, const int64_t* rows_a, const int64_t* rows_b, long N, int D, long V, long L,
                            float* out, void* stream);

/* ---- majority vote -------------------------------------------------------------------------------------------------------
 * argmin[v]  = the d with active[d] != 0 and the smallest stat[v,d] (ties: the lowest d; a NaN is never chosen), -1 when no
 *              dimension is active or every active statistic is NaN
 * votes[k,d] = #{v : factor[v] == k and argmin[v] == d}            (every element written, zeros included)
 * stat fp32 [V,D]; factor int32 [V], every entry in [0, K) -- the CALLER checks that; active int32 [D] (0 / 1);
 * argmin int32 [V]; votes int32 [K,D].                                                                                    */
int dvae_score_vote(const float* stat, const int32_t* factor, const int32_t* active, long V, int D, int K, int32_t* argmin,
                    int32_t* votes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
