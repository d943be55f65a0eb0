/*
 * libdvae_sap_hip.so -- C-ABI of the MI355X (gfx950) kernels behind Evaluator.compute_sap_discrete: the SAP score (Kumar et al.
 * 2018) with DISCRETE factors, the branch of disentanglement_lib's sap_score.py that its shipped configuration selects
 * (sap_score.continuous_factors = False).  Entry [d, k] of the score matrix is the test accuracy of
 * LinearSVC(C = 0.01, class_weight = "balanced") fitted on ONE latent as its only feature.  With one feature a one-vs-rest
 * squared-hinge SVM is a strictly convex, piecewise-quadratic problem in two unknowns, and Newton's method on the active set
 * reaches its exact minimiser: every (latent, factor, class) problem is fitted here, on the device, in one launch.
 * A thirteenth library next to libdvae_hip.so (include/dvae_hip.h): nothing here is part of the training step and nothing here is
 * recorded into a launch plan.  The reference (YannDubs/disentangling-vae) has no counterpart.
 *
 * Conventions, as in dvae_info_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (fp64 / int64 / int32 where stated), aligned to its element size and no more,
 *     except n_classes, which is a HOST pointer read during the call; sizes are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation); there is no
 *     workspace: a problem lives in the LDS of its workgroup;
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_sap_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - no atomics, no cooperative launch, no workgroup waits on another: every thread adds its rows in a fixed order and the
 *     partial sums are combined in a fixed tree, the same inputs give the same bits;
 *   - the table is fp32, everything else is fp64.
 *
 * table: fp32 [N, D], one ROW per data point (the posterior means in data-set order), any D in [1, DVAE_SAP_MAX_D].
 * rows: int64 row numbers, every entry in [0, N) -- the CALLER checks that, the device does not -- repeats allowed.
 * n_classes: HOST int32 [K], the number of classes PRESENT in the training rows of every factor, each in
 * [1, DVAE_SAP_MAX_CLASSES]; labels of factor j are the ranks 0 .. n_classes[j] - 1 of its values among those present.
 * A factor with C_j >= 3 classes has C_j problems (class k against the rest), one with 2 classes has ONE problem (class 1 against
 * class 0), one with 1 class has none: P = dvae_sap_problems(n_classes, K) problems per latent, in the order of the factors and,
 * within a factor, of the classes.
 */
#ifndef DVAE_SAP_HIP_H
#define DVAE_SAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_SAP_VERSION 1

/* limits: K above DVAE_SAP_MAX_FACTORS, a factor with more than DVAE_SAP_MAX_CLASSES classes present and D above
 * DVAE_SAP_MAX_D are refused                                                                                               */
#define DVAE_SAP_MAX_FACTORS 8
#define DVAE_SAP_MAX_CLASSES 256
#define DVAE_SAP_MAX_D 65535
/* One workgroup of DVAE_SAP_THREADS threads owns one problem.  It gathers its column of the table (fp32) and the side of every
 * row (one byte) ONCE into LDS and iterates there: 5 bytes of LDS per training row, so DVAE_SAP_MAX_ROWS = 16384 rows take
 * 80 KiB of the 160 KiB of a compute unit (10 000 rows, disentanglement_lib's figure, and the 10 240 of DCI: three and two
 * workgroups per compute unit).  There is NO second path that reads the column from a workspace: more training rows than
 * DVAE_SAP_MAX_ROWS are an invalid argument of dvae_sap_fit (the Python side raises ValueError before any device work).
 * dvae_sap_accuracy keeps no row in LDS and takes any number of rows.                                                       */
#define DVAE_SAP_THREADS 256
#define DVAE_SAP_MAX_ROWS 16384
/* Newton's method takes at most DVAE_SAP_MAX_ITERATIONS steps, each of them at most DVAE_SAP_MAX_HALVINGS halvings of the step
 * (bounded loops both); the problems tried so far took 14 steps or fewer.  A problem that reaches the first bound reports
 * iterations = -1.                                                                                                         */
#define DVAE_SAP_MAX_ITERATIONS 64
#define DVAE_SAP_MAX_HALVINGS 30

int dvae_sap_version(void);
const char* dvae_sap_last_error(void);

/* P: sum over the factors of (C_j if C_j >= 3, 1 if C_j == 2, 0 if C_j == 1); -1 when K or a C_j is out of range.            */
long dvae_sap_problems(const int32_t* n_classes, int K);

/* ---- the fit ------------------------------------------------------------------------------------------------------------------
 * rows int64 [S] (the training rows), labels int32 [K, S]: labels[j, i] in [0, n_classes[j]) is the class of factor j in
 * training row i (the CALLER checks the range; every class of a factor must occur).  For latent d and the problem of class k of
 * factor j, with x_i = table[rows[i], d], s_i = +1 where labels[j, i] == k and -1 elsewhere, the objective of
 * LinearSVC(C, class_weight = "balanced") (liblinear's L2-regularised L2-loss SVC with a regularised intercept) is
 *   f(w, b) = (w^2 + b^2) / 2 + sum_i c_i max(0, 1 - s_i (w x_i + b))^2
 *   C_j >= 3:  c_i = C S / (C_j count_k) for s_i = +1 and c_i = C for s_i = -1     (liblinear weighs the positives only)
 *   C_j == 2:  k = 1;  c_i = C S / (2 count_1) for s_i = +1 and c_i = C S / (2 count_0) for s_i = -1
 * count_k = the number of training rows of class k, counted HERE: no weight is passed in.
 * Newton's method from (0, 0).  With A = {i : s_i (w x_i + b) < 1} the active rows at the current point and
 *   S1 = sum_A c_i, Sx = sum_A c_i x_i, Sxx = sum_A (c_i x_i) x_i, Rx = sum_A (c_i s_i) x_i, R1 = sum_A c_i s_i
 * the FULL step goes to the minimiser of the quadratic piece of A:
 *   a = 1 + 2 Sxx, h = 2 Sx, e = 1 + 2 S1, det = a e - h h;   w' = (e 2 Rx - h 2 R1) / det,  b' = (a 2 R1 - h 2 Rx) / det.
 * It STOPS when the active set at (w', b') is A: (w', b') is then the exact minimiser of f, and `iterations` is the number of
 * full steps computed.  Otherwise the step t = 1, 1/2, 1/4, ... (at most DVAE_SAP_MAX_HALVINGS halvings) is the first whose
 * point theta + t (theta' - theta) has an objective BELOW the current one; when none has, the current point is kept as the
 * minimiser (no point along a descent direction of a convex function lowers it: it is the minimiser to rounding).  That exit is
 * what a row exactly ON the hinge at the optimum takes: the minimisers of the two pieces that meet there are one point in exact
 * arithmetic and two neighbours in fp64, and the full step hops from one to the other without lowering the objective.
 * Outputs: coef fp64 [D, P, 2] (w, b), iterations int32 [D, P] (>= 1; -1 after DVAE_SAP_MAX_ITERATIONS steps without a stop, or
 * for a class that no training row carries -- coef is then (0, 0)); every element is written.  P = 0 enqueues nothing.
 * 1 <= S <= DVAE_SAP_MAX_ROWS, C > 0 and finite, N <= 2^31 - 1.                                                                */
int dvae_sap_fit(const float* table, const int64_t* rows, const int32_t* labels, const int32_t* n_classes, long N, int D, int K,
                 long S, double C, double* coef, int32_t* iterations, void* stream);

/* ---- the accuracy -------------------------------------------------------------------------------------------------------------
 * rows int64 [T], labels int32 [K, T]: the class of factor j in row i, or -1 for a value that the training rows do not hold --
 * such a row counts as an error.  coef as dvae_sap_fit writes it.  For latent d, factor j and x = table[rows[i], d] the decision
 * value of class k is  fl(fl(w_k x) + b_k)  in fp64: the product ROUNDED, then the sum -- never a fused multiply-add.
 *   C_j >= 3: the class with the largest decision value, the lowest such class on ties;
 *   C_j == 2: class 1 where the decision value of the one problem is > 0, else class 0;
 *   C_j == 1: class 0.
 * Outputs: correct int32 [D, K], the number of rows whose predicted class is their label; predicted int32 [D, K, T], or NULL.
 * Every element is written.  1 <= T <= 2^31 - 1.                                                                               */
int dvae_sap_accuracy(const float* table, const int64_t* rows, const int32_t* labels, const int32_t* n_classes, long N, int D,
                      int K, long T, const double* coef, int32_t* correct, int32_t* predicted, void* stream);

#ifdef __cplusplus
}
#endif
#endif
