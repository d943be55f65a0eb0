/*
 * libdvae_udr_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the unsupervised disentanglement ranking of
 * Evaluator.compute_udr (Duan et al. 2020; disentanglement_lib's udr.py): the tie-averaged rank transform of every column of a
 * table of posterior means -- a segmented radix sort, what the Spearman form of UDR correlates -- and the mean KL divergence of
 * every latent dimension from the prior, which tells the informative latents from the collapsed ones.  A seventh library next to
 * libdvae_hip.so (include/dvae_hip.h), libdvae_eval_hip.so, libdvae_score_hip.so, libdvae_info_hip.so, libdvae_irs_hip.so and
 * libdvae_unsup_hip.so (include/dvae_unsup_hip.h, whose dvae_unsup_moments correlates the rank tables): nothing here is part
 * of the training step and nothing here is recorded into a launch plan.  The reference (YannDubs/disentangling-vae) has no
 * counterpart.
 *
 * Conventions, as in dvae_unsup_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (fp64 / int64 where stated), aligned to its element size and no more;
 *     sizes are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation);
 *     workspace is caller-provided and needs no initialisation;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_udr_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - the ranks are counted, not summed, and the one floating-point reduction (the KL) has a fixed order; there are no float
 *     atomics: the same inputs give the same bits.
 *
 * table / mean / logvar: fp32 [N, D], one ROW per data point, 1 <= D <= DVAE_UDR_MAX_D.
 * rows: int64 [S] row numbers, every entry in [0, N) -- the CALLER checks that, the device does not -- repeats allowed; or
 * NULL: all N rows in order (S is then ignored and taken as N).  N is at most 2^31 - 1.
 */
#ifndef DVAE_UDR_HIP_H
#define DVAE_UDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_UDR_VERSION 1

/* limits: D above DVAE_UDR_MAX_D is refused; the ranks refuse more than DVAE_UDR_MAX_ROWS selected rows (2^23: up to there
 * every half-integer rank (first + last) / 2 + 1 <= 2^23 is an fp32 number)                                                  */
#define DVAE_UDR_MAX_D 64
#define DVAE_UDR_MAX_ROWS 8388608
/* ranks: up to DVAE_UDR_SMALL_ROWS selected rows one workgroup sorts a column in LDS (one launch).  Above, a column is cut
 * into equal chunks, one workgroup per (chunk, column): ceil(S / DVAE_UDR_CHUNK_ROWS) of them, at most DVAE_UDR_MAX_CHUNKS --
 * from there on the chunks grow instead -- and every radix pass is three launches over ping-pong buffers in ws.               */
#define DVAE_UDR_SMALL_ROWS 2048
#define DVAE_UDR_CHUNK_ROWS 2048
#define DVAE_UDR_MAX_CHUNKS 256
/* KL: one THREAD per (chunk of rows, latent) adds its rows in order, so the chunks are short and many:
 * ceil(S / DVAE_UDR_KL_BLOCK_ROWS) chunks, at most DVAE_UDR_KL_MAX_CHUNKS, then they grow.                                  */
#define DVAE_UDR_KL_BLOCK_ROWS 64
#define DVAE_UDR_KL_MAX_CHUNKS 4096

int dvae_udr_version(void);
const char* dvae_udr_last_error(void);

/* ---- tie-averaged ranks of every column --------------------------------------------------------------------------------------
 * x_s = table[rows[s], :], s < S <= DVAE_UDR_MAX_ROWS:
 *   ranks[s, d]   fp32 [S, D] = #{t : x_td < x_sd} + (#{t : x_td == x_sd} + 1) / 2
 * the 1-based average rank of x_sd among x_.d (scipy.stats.rankdata(method="average")), EXACT: comparison is the numeric
 * comparison of the fp32 values -- -0.0 and +0.0 tie, negatives order below positives, denormals are not flushed -- and a row
 * selected twice ties with itself.  The table must be finite (the CALLER checks that).  Every element of ranks is written.
 * Every value becomes an order-preserving 32-bit key; (key, s) is sorted per column by an LSD radix sort of 8-bit digits --
 * digit counts per (column, chunk), an exclusive scan to offsets, a stable scatter; launch boundaries are the only ordering
 * between workgroups -- and every run of equal keys [first, last] of the sorted column gives (first + last) / 2 + 1 to its rows.
 * ws: dvae_udr_ranks_ws_floats(N, D, S) floats (S <= 0: as for NULL rows; 0 for sizes out of range, 1 or more otherwise):
 * 4 S D for the ping-pong buffers above DVAE_UDR_SMALL_ROWS, plus the counters.                                              */
size_t dvae_udr_ranks_ws_floats(long N, int D, long S);
int dvae_udr_ranks(const float* table, const int64_t* rows, long N, int D, long S, float* ws, float* ranks, void* stream);

/* ---- KL divergence per latent dimension -------------------------------------------------------------------------------------
 * mu_s = mean[rows[s], :], lv_s = logvar[rows[s], :], s < S <= 2^31 - 1:
 *   kl[d]   fp64 [D] = (1 / S) sum_s 0.5 (mu_sd^2 + exp(lv_sd) - lv_sd - 1)
 * every element converted to fp64 BEFORE any arithmetic; the rows of a chunk are added in order, the chunks in order; kl is
 * fp64 and is never rounded to fp32.
 * ws: dvae_udr_kl_dims_ws_floats(N, D, S) floats (S <= 0: as for NULL rows; 0 for sizes out of range).                        */
size_t dvae_udr_kl_dims_ws_floats(long N, int D, long S);
int dvae_udr_kl_dims(const float* mean, const float* logvar, const int64_t* rows, long N, int D, long S, float* ws, double* kl,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
