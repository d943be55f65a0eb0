/*
 * libdvae_knn_hip.so -- C-ABI of the MI355X (gfx950) kernels behind Evaluator.compute_knn_information_scores: the BINNING-FREE
 * mutual information between one continuous latent and one discrete factor of variation, by the k-nearest-neighbour estimator
 * of Ross 2014 (the Kraskov family; scikit-learn's sklearn.feature_selection._mutual_info._compute_mi_cd), for every
 * (latent, factor) pair of a table of posterior means.  MIG, modularity, MIG-sup, DCIMIG and the InfoMEC scores InfoM and InfoC
 * (Hsu et al. 2023) are combined from the [latent, factor] matrix on the host.
 * A fourteenth library next to libdvae_hip.so (include/dvae_hip.h): nothing here is part of the training step and nothing here is
 * recorded into a launch plan.  The reference (YannDubs/disentangling-vae) has no counterpart.
 *
 * The estimator.  x[0..S) is one fp32 latent column of the selected rows, v[0..S) the value of one factor in them,
 * kn = n_neighbors >= 1.  For row i: c_i = the number of selected rows with v == v_i.  Rows with c_i == 1 are dropped from
 * everything below; n rows are kept.  k_i = min(kn, c_i - 1).  r_i = the k_i-th smallest |x_j - x_i| over the OTHER kept rows j
 * with v_j == v_i (a duplicate value is at distance 0, a repeated row is another row).  r_i > 0: m_i = the number of kept rows j,
 * i included, with |x_j - x_i| < r_i, strictly.  r_i == 0: m_i = the number of kept rows with x_j == x_i.  Differences are taken
 * after conversion to fp64; -0 equals +0; denormals are kept.  Then
 *   raw = psi(n) + mean_i psi(k_i) - mean_i psi(c_i) - mean_i psi(m_i),   I = max(0, raw),   I = 0 where n == 0
 * with psi the digamma function.  The device returns the integers and the three SUMS; psi(n), the means, the clipping and the
 * scores are the host's.  scikit-learn's `nextafter(r, 0)` with `<=` is the strict `<` here.
 *
 * Conventions, as in dvae_sap_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (fp64 / int64 / int32 where stated), aligned to its element size and no more,
 *     except lat_sizes, which is a HOST pointer read during the call; sizes are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation); the caller owns the
 *     workspace: dvae_knn_ws_bytes bytes, written by dvae_knn_sort and read by dvae_knn_mi on the same stream;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_knn_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - no atomics on floats (class counts are integer adds in LDS), no cooperative launch, no workgroup waits on another, bounded
 *     loops only: every thread adds its rows in a fixed order and the partial sums are combined in a fixed tree, the same inputs
 *     give the same bits;
 *   - the table is fp32, the sums are fp64, everything between is integer-exact.
 *
 * table: fp32 [N, D], one ROW per data point of a data set that ENUMERATES lat_sizes in row-major order: N = prod(lat_sizes) and
 * the value of factor k in row r is (r / stride_k) % lat_sizes[k], stride_k = prod(lat_sizes[k + 1 ..]).  Labels never exist in
 * memory.  rows: int64 [S] row numbers, every entry in [0, N) -- the CALLER checks that, the device does not -- repeats allowed;
 * NULL: every row (S = N).  lat_sizes: HOST int32 [K], each in [1, DVAE_KNN_MAX_CLASSES].
 */
#ifndef DVAE_KNN_HIP_H
#define DVAE_KNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_KNN_VERSION 1

/* limits: K above DVAE_KNN_MAX_FACTORS, a factor with more than DVAE_KNN_MAX_CLASSES values, n_neighbors above
 * DVAE_KNN_MAX_NEIGHBORS and D above DVAE_KNN_MAX_D (= DVAE_SAP_MAX_D) are refused                                            */
#define DVAE_KNN_MAX_FACTORS 8
#define DVAE_KNN_MAX_CLASSES 256
#define DVAE_KNN_MAX_NEIGHBORS 64
#define DVAE_KNN_MAX_D 65535
/* A column lives in the LDS of ONE workgroup in both kernels; there is NO second path: more selected rows than
 * DVAE_KNN_MAX_ROWS are an invalid argument (the Python side raises ValueError before any device work).
 * dvae_knn_sort: DVAE_KNN_SORT_THREADS threads, one 8-byte (key, selection index) pair per row of the column padded to a power of
 * two: 128 KiB at 16 384 rows.
 * dvae_knn_mi: DVAE_KNN_MI_THREADS threads, DVAE_KNN_MI_ROW_BYTES bytes per row (the value fp32, its place in the compacted list
 * uint16 per class-list entry, the selection index uint16, the label uint8) plus DVAE_KNN_MI_FIXED_BYTES of tables:
 * 9 * 16 384 + 11 520 = 158 976 bytes of the 160 KiB of a compute unit.                                                       */
#define DVAE_KNN_MAX_ROWS 16384
#define DVAE_KNN_SORT_THREADS 1024
#define DVAE_KNN_SORT_ROW_BYTES 8
#define DVAE_KNN_MI_THREADS 512
#define DVAE_KNN_MI_ROW_BYTES 9
#define DVAE_KNN_MI_FIXED_BYTES 11520

int dvae_knn_version(void);
const char* dvae_knn_last_error(void);

/* Bytes of the workspace of both entry points for S selected rows (S <= 0: every row, S = N) of D latents: the sorted values
 * fp32 [D, S], then their selection indices int32 [D, S].  0 when a size is out of range.                                     */
size_t dvae_knn_ws_bytes(long N, int D, long S);

/* ---- the sort -----------------------------------------------------------------------------------------------------------------
 * One workgroup per latent column d gathers x_s = table[rows[s], d], s in [0, S), and sorts the pairs (key(x_s), s) ascending,
 * key being the 32-bit word whose unsigned order is the numeric order of the floats (+0 and -0 one key).  Equal values lie in
 * the order of s, and no output of dvae_knn_mi depends on the order among equal values.  Outputs, in ws: the sorted values
 * (a -0 is written as +0) and the selection index of each.  1 <= S <= DVAE_KNN_MAX_ROWS, N <= 2^31 - 1.                        */
int dvae_knn_sort(const float* table, const int64_t* rows, long N, int D, long S, void* ws, void* stream);

/* ---- the estimator ------------------------------------------------------------------------------------------------------------
 * One workgroup per (latent d, factor k) takes column d's sorted list from ws (as dvae_knn_sort left it: same table, rows, N, D
 * and S), forms every row's label from its ROW NUMBER, counts the classes, drops the rows of singleton classes by a stable
 * compaction, splits the sorted list stably by class (every class list is itself sorted), finds r_i by an outward walk of at
 * most k_i steps in its class list and m_i by two binary searches in the compacted full list on exact fp64 differences, and adds
 * psi[k_i], psi[c_i] and psi[m_i] in fp64 in a fixed order.
 * psi: fp64 [S + 1], psi[j] = digamma(j) for j in [1, S], built on the host; entry 0 is never read.
 * Outputs: sums fp64 [D, K, 4] = (n, sum psi(k_i), sum psi(c_i), sum psi(m_i)) over the kept rows; class_counts int32
 * [K, sum_sizes], sum_sizes = sum(lat_sizes): row k holds the counts of factor k's values among ALL S selected rows in the
 * columns [sum(lat_sizes[..k]), + lat_sizes[k]) and 0 in every other column; m_of / k_of int32 [D, K, S] or NULL: m_i and k_i by
 * SELECTION index, 0 for a dropped row.  Every element is written.
 * 1 <= n_neighbors <= DVAE_KNN_MAX_NEIGHBORS, prod(lat_sizes) == N.                                                            */
int dvae_knn_mi(const int64_t* rows, const int32_t* lat_sizes, long N, int D, int K, long S, int n_neighbors, const double* psi,
                const void* ws, double* sums, int32_t* class_counts, int32_t* m_of, int32_t* k_of, void* stream);

#ifdef __cplusplus
}
#endif
#endif
