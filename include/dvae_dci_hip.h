/*
 * libdvae_dci_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the DCI scores of Evaluator.compute_dci (Eastwood & Williams
 * 2018 in disentanglement_lib's form, dci.py): gradient-boosted depth-3 regression trees -- scikit-learn's
 * GradientBoostingClassifier with default arguments, restated -- fitted on a table of posterior means, their impurity-based
 * feature importances and their raw scores on held-out rows.  An eighth library next to libdvae_hip.so (include/dvae_hip.h),
 * libdvae_eval_hip.so, libdvae_score_hip.so, libdvae_info_hip.so, libdvae_irs_hip.so, libdvae_unsup_hip.so and
 * libdvae_udr_hip.so: nothing here is part of the training step and nothing here is recorded into a launch plan.  The reference
 * (YannDubs/disentangling-vae) has no counterpart.
 *
 * Conventions, as in dvae_udr_hip.h:
 *   - every pointer is a DEVICE pointer, aligned to its element size and no more (fp32 4, int32 4, fp64 / int64 8); `ws` is
 *     sized in floats and aligned to 8 bytes; sizes are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation, no read-back
 *     between stages or levels); workspace is caller-provided and needs no initialisation;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_dci_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - the table is fp32, everything else is fp64 in a FIXED summation order (below); there are no float atomics and no
 *     workgroup waits on another (launch boundaries are the only ordering): the same inputs give the same bits.
 *
 * table: fp32 [N, D], one ROW per data point, 1 <= D <= DVAE_DCI_MAX_D, finite (the CALLER checks that).
 * rows: int64 [S] row numbers, every entry in [0, N) -- the CALLER checks that, the device does not -- repeats allowed; or
 * NULL: all N rows in order (S is then ignored and taken as N).  1 <= S <= DVAE_DCI_MAX_ROWS, N <= 2^31 - 1.
 * x_s = table[rows[s], :] is selected row s.
 * labels: int32 [S] in [0, C) -- the CALLER checks that --, 1 <= C <= DVAE_DCI_MAX_CLASSES.
 * T = trees per stage = dvae_dci_trees(C): C, or 1 for C <= 2 (two classes share one tree; one class is the degenerate case:
 * its residuals are zero, no tree splits, the importances are zero).
 *
 * The model (scikit-learn 1.7's GradientBoostingClassifier(): log loss, learning rate 0.1, 100 stages, friedman_mse, depth 3,
 * min_samples_split 2, min_samples_leaf 1, no subsampling):
 *   prior        q_k = clip(#{labels = k} / S, e, 1 - e), e = 2^-23;  C >= 3: raw_k = log(q_k / exp(mean_j log q_j));
 *                C = 2: raw_0 = log(q_1 / (1 - q_1));  C = 1: raw_0 = 0.
 *   stage        p = softmax(raw_s) (C = 2: p = 1 / (1 + exp(-raw_s))) from the raw scores BEFORE the stage, for all T trees;
 *                residual of tree k: r_s = [labels_s = k] - p_sk (C = 2: labels_s - p_s).
 *   tree         15 nodes in heap order (children of h: 2 h + 1, 2 h + 2).  A node with n rows, sum r and sum r^2 is a leaf when
 *                it is at depth 3, n < 2, sum r^2 / n - (sum r / n)^2 <= 2^-52, or no candidate exists.  Candidates of feature d: in
 *                the stable ascending order of x_.d, every row of the node whose value exceeds that of the node's row before it
 *                by more than 1e-7 (fp32 addition and comparison); gain = (nR SL - nL SR)^2 / (nL nR) with nL, SL the count
 *                and residual sum of the node's rows before it, SR = sum r - SL; threshold = lo / 2 + hi / 2 in fp64 (lo if that
 *                equals hi or is infinite); rows with (double)x <= threshold go left.  The largest gain wins; among EXACTLY
 *                equal gains the lowest feature, then the lowest position (scikit-learn visits the features in an order
 *                drawn from random_state and keeps the first of equal gains: a stated difference).
 *   leaf value   f (sum r / n) / (sum h / n), h = p (1 - p) with p = y - r, f = (C - 1) / C (C = 2: 1); 0 when |sum h / n| < 1e-150;
 *                raw_sk += learning_rate * value of the leaf of x_s.  The value of an inner node is sum r / n.
 *   importance   of feature d in one tree: sum over the inner nodes that split on d of (n mse - nL mseL - nR mseR) / S,
 *                mse = sum r^2 / n - (sum r / n)^2 -- NOT normalised per tree: GradientBoostingClassifier.feature_importances_
 *                averages these over the trees with more than one node and normalises once.
 * Summation order.  Node statistics (n, sum r, sum r^2, sum h): thread t of DVAE_DCI_THREADS adds the selected rows
 * [t c, (t + 1) c), c = ceil(S / DVAE_DCI_THREADS), in order; the 64 lanes of a wave are added pairwise at distances 32, 16, ...,
 * 1; the waves in order.  Split search of one (tree, feature): thread t walks positions [t c, (t + 1) c) of the sorted column;
 * the prefix (count, sum r, last value) per open node of the threads before it is an in-workgroup scan -- within a wave by
 * doubling distances 1, 2, ..., 32, then the waves before in order -- and the thread adds its own rows to it in order.
 */
#ifndef DVAE_DCI_HIP_H
#define DVAE_DCI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_DCI_VERSION 1

/* limits: sizes above are refused.  DVAE_DCI_MAX_ROWS is what one workgroup holds of a sorted column in LDS:
 * DVAE_DCI_ROW_LDS_BYTES per row (residual fp64, value fp32, node byte) plus DVAE_DCI_LDS_SCRATCH for the scan, within the
 * 160 KB of a CDNA4 compute unit.                                                                                           */
#define DVAE_DCI_MAX_D 64
#define DVAE_DCI_MAX_CLASSES 256
#define DVAE_DCI_MAX_ROWS 10240
#define DVAE_DCI_MAX_STAGES 1024
#define DVAE_DCI_THREADS 1024
#define DVAE_DCI_ROW_LDS_BYTES 13
#define DVAE_DCI_LDS_SCRATCH 4096
/* a tree is DVAE_DCI_NODES nodes; tree_stats holds DVAE_DCI_NODE_STATS doubles per node                                     */
#define DVAE_DCI_NODES 15
#define DVAE_DCI_NODE_STATS 5
/* launches of one stage: residuals, root statistics, then (search, split) for the levels 0, 1, 2                            */
#define DVAE_DCI_LAUNCHES_PER_STAGE 8

int dvae_dci_version(void);
const char* dvae_dci_last_error(void);
/* T: trees per stage and columns of `raw` (0 for C out of range) */
int dvae_dci_trees(int C);

/* ---- fit ----------------------------------------------------------------------------------------------------------------------
 * order: int32 [D, S], order[d, i] = the selected row (an index into [0, S)) at position i of the STABLE ascending order of
 *   x_.d -- torch.sort(table[rows], dim=0, stable=True) transposed; the CALLER provides it (once per table, for all factors).
 * raw: fp64 [S, T], in / out.  init != 0: the call first sets every row to the prior of `labels`; init == 0: it continues from
 *   what is there (the raw scores an earlier call left: n1 + n2 stages in two calls give the bits of n1 + n2 in one).
 * prior: fp64 [T], out: the prior raw scores of `labels` (above), the same for every row -- what dvae_dci_predict starts from;
 *   written whatever `init` is.
 * importance: fp64 [D], the sum over this call's n_stages * T trees, in order, of the per-tree importances (above);
 * n_split: int32 [1], how many of them split at all.
 * tree_feature: int32 [n_stages, T, 15]: the feature a node splits on, -1 for a leaf and for a node that does not exist.
 * tree_stats: fp64 [n_stages, T, 15, 5]: threshold (0 unless the node splits), value, n (0: the node does not exist), sum r,
 *   sum r^2.  Every element of every output is written.
 * ws: dvae_dci_fit_ws_floats(N, D, S, C, n_stages) floats (S <= 0: as for NULL rows; 0 for sizes out of range), 8-byte aligned. */
size_t dvae_dci_fit_ws_floats(long N, int D, long S, int C, int n_stages);
int dvae_dci_fit(const float* table, const int64_t* rows, const int32_t* order, const int32_t* labels, long N, int D, long S, int C,
                 int n_stages, double learning_rate, int init, double* raw, double* prior, float* ws, double* importance,
                 int32_t* n_split, int32_t* tree_feature, double* tree_stats, void* stream);

/* ---- predict ------------------------------------------------------------------------------------------------------------------
 * raw fp64 [S, T], in / out: raw_sk += learning_rate * value of the leaf of x_s in tree k of stage i, for the stages in order
 * (the caller fills it with the prior first).  No workspace.  On the rows of the fit it gives the bits the fit left in `raw`.  */
int dvae_dci_predict(const float* table, const int64_t* rows, long N, int D, long S, int C, int n_stages, double learning_rate,
                     const int32_t* tree_feature, const double* tree_stats, double* raw, void* stream);

#ifdef __cplusplus
}
#endif
#endif
