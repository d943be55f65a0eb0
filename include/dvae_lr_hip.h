/*
 * libdvae_lr_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the linear-softmax probes of the Evaluator: the multinomial
 * logistic regression of the beta-VAE score and of explicitness (evaluate.py's fit_logistic_regression, scikit-learn's default
 * objective) and of InfoE (Hsu et al. 2023), FITTED ON THE DEVICE by a truncated Newton-CG iteration in fp64, and the evaluation
 * of the fits (probabilities, log-loss, accuracy).  A fifteenth library next to libdvae_hip.so (include/dvae_hip.h): nothing here
 * is part of the training step and nothing here is recorded into a launch plan.  The reference (YannDubs/disentangling-vae) has no
 * counterpart.
 *
 * Conventions, as in dvae_sap_hip.h:
 *   - every pointer is a DEVICE pointer to fp32 (fp64 / int32 where stated), aligned to its element size and no more (`ws` to 8
 *     bytes), except n_classes, which is a HOST pointer read during the call; sizes are element counts;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work (no allocation, no synchronisation);
 *   - return 0 on success, <0 on invalid argument / launch error (text via dvae_lr_last_error(), per thread); argument
 *     errors are reported before any launch;
 *   - no float atomics, no cooperative launch, no workgroup waits on another: every sum is added in a fixed order (stated
 *     below), the same inputs give the same bits;
 *   - the features are fp32, everything else is fp64; nothing is read back between iterations: a whole solve is ONE launch.
 *
 * features: fp32 [S, D] (the caller gathers the rows: that is plumbing), 1 <= D <= DVAE_LR_MAX_D.
 * shift, scale: fp64 [D], or BOTH NULL.  When given, x_d = fl(fl((double)feature_d - shift_d) * scale_d), formed in fp64; when
 * NULL, x_d = (double)feature_d.  A column with scale_d = 0 is the constant 0: its weights stay exactly 0.
 * n_classes: HOST int32 [Q], the classes C_q of every problem, each in [1, DVAE_LR_MAX_CLASSES]; 1 <= Q <= DVAE_LR_MAX_PROBLEMS.
 * The Q problems share the feature matrix and differ in their labels.
 * coef: fp64, per problem C_q (D + 1) values -- W [C_q, D] row-major, then b [C_q] -- packed in problem order.
 */
#ifndef DVAE_LR_HIP_H
#define DVAE_LR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_LR_VERSION 1

/* limits: more is an invalid argument (the Python side raises ValueError before any device work)                              */
#define DVAE_LR_MAX_ROWS 16384
#define DVAE_LR_MAX_D 64
#define DVAE_LR_MAX_CLASSES 256
#define DVAE_LR_MAX_PROBLEMS 8
/* One persistent workgroup of DVAE_LR_THREADS threads owns one problem and runs its whole solve.  The probabilities of the
 * training rows do not fit in LDS (S C 8 bytes): they, the iteration's vectors and the chunk partials live in `ws`.
 * A pass over the rows (thread t takes rows t, t + DVAE_LR_THREADS, ...) forms the logits DVAE_LR_FEATURE_TILE features at a
 * time -- b_c first, then the products in ascending d -- and the softmax of every row.  A sum over the rows (the gradient, a
 * Hessian-vector product) is split into n_chunks = min(DVAE_LR_THREADS / (C (D + 1)) (at least 1), ceil(S / DVAE_LR_CHUNK_ROWS))
 * chunks of ceil(S / n_chunks) consecutive rows; every (chunk, entry) partial is added in row order by one thread, and the
 * partials of an entry are added in chunk order.  A sum over the entries of a vector or over the per-row losses: thread t adds
 * its elements t, t + DVAE_LR_THREADS, ... in that order, the 64 lanes of a wave by a fixed shuffle tree, the waves in their
 * order.                                                                                                                    */
#define DVAE_LR_THREADS 512
#define DVAE_LR_FEATURE_TILE 16
#define DVAE_LR_CHUNK_ROWS 64
/* dvae_lr_predict: one workgroup of DVAE_LR_PREDICT_THREADS threads per problem walks all T rows.                              */
#define DVAE_LR_PREDICT_THREADS 128
/* The bounds of the solver's three loops: outer Newton iterations, conjugate-gradient steps of one of them, halvings of one
 * step.  A problem that reaches the first without meeting tolerance_grad (or finds no acceptable step) reports -1.          */
#define DVAE_LR_MAX_ITERATIONS 100
#define DVAE_LR_MAX_CG 400
#define DVAE_LR_MAX_HALVINGS 30

int dvae_lr_version(void);
const char* dvae_lr_last_error(void);

/* Bytes of the workspace of dvae_lr_fit for these sizes, or -1 when an argument is out of range (S in [1, DVAE_LR_MAX_ROWS],
 * D in [1, DVAE_LR_MAX_D], Q in [1, DVAE_LR_MAX_PROBLEMS], every C_q in [1, DVAE_LR_MAX_CLASSES]).  Per problem, in doubles:
 * 2 C_q S (probabilities, row products) + n_chunks C_q (D + 1) (chunk partials) + 8 C_q (D + 1) (the iteration's vectors).    */
long dvae_lr_ws_bytes(long S, int D, const int32_t* n_classes, int Q);

/* ---- the fit ------------------------------------------------------------------------------------------------------------------
 * labels int32 [Q, S]: labels[q, i] in [0, n_classes[q]) (the CALLER checks the range).  Problem q minimises over
 * theta = (W [C_q, D], b [C_q])
 *   f(theta) = (1 / S) sum_i ( logsumexp_c(W_c . x_i + b_c) - (W_{y_i} . x_i + b_{y_i}) ) + ||W||^2 / (2 C S)
 * -- the bias is unpenalised; this is fit_logistic_regression's objective and scikit-learn's default -- from theta = 0.
 * f is strictly convex in W and invariant to adding one constant to every b_c.  THE SOLVER STAYS ON sum_c b_c = 0: it starts
 * there, the bias gradient sums to zero, and every step is a combination of gradients and Hessian-vector products of such
 * vectors, whose bias parts sum to zero too (in fp64: to rounding; compare b after centring).
 * Truncated Newton-CG.  With g the gradient at theta and H v = (1 / S) X^T (diag(p) - p p^T) X v + (v_W / (C S), 0) the
 * Hessian-vector product (one pass over the rows and one sum over them, the cost of a gradient):
 *   stop          when max |g| <= tolerance_grad: `iterations` = the steps taken so far;
 *   direction     conjugate gradients on H s = -g from s = 0, preconditioned by the diagonal of H ((1 / S) sum_i p_ic (1 - p_ic) x_id^2
 *                 + 1 / (C S); one more sum over the rows per step; the C biases share ONE number, the mean of their entries,
 *                 because unequal ones would take the direction off sum_c b_c = 0), at most DVAE_LR_MAX_CG steps, until
 *                 ||residual||_2 <= min(0.5, sqrt(||g||_2)) ||g||_2 (or a direction without curvature);
 *   step          t = 1, 1/2, ... (at most DVAE_LR_MAX_HALVINGS halvings), the first with
 *                 f(theta + t s) <= f(theta) + 1e-4 t g.s, or with f no more than 1e-12 |f| above f(theta) and a smaller max |g|
 *                 (near the optimum the decrease of f is below its rounding); every trial is one function evaluation (f and g).
 * At most DVAE_LR_MAX_ITERATIONS steps.
 * Outputs: coef (above); report fp64 [Q, 4] = (f, max |g| at the returned point -- both as the device computed them --,
 * steps taken or -1 where the solve stopped without meeting tolerance_grad, function evaluations).  Every element of both is
 * written.  C > 0 and finite, tolerance_grad >= 0 and finite, ws: dvae_lr_ws_bytes(S, D, n_classes, Q) bytes, 8-byte aligned. */
int dvae_lr_fit(const float* features, const double* shift, const double* scale, const int32_t* labels, const int32_t* n_classes,
                long S, int D, int Q, double C, double tolerance_grad, void* ws, double* coef, double* report, void* stream);

/* ---- the evaluation of the fits -------------------------------------------------------------------------------------------------
 * features fp32 [T, D], labels int32 [Q, T]: the class of row i in problem q, or -1 for a value that the training rows do not
 * hold -- such a row is left out of log_loss / counted and counts as an error in correct.  coef as dvae_lr_fit writes it.
 * The logits are b_c + sum_d W_cd x_d in ascending d, in fp64; the predicted class is the arg-max, the lowest class on ties.
 * Outputs: prob fp32, per problem [T, C_q] packed in problem order, or NULL: exp(z_c - max z) / sum_c' exp(z_c' - max z) formed
 * in fp64 and rounded once; log_loss fp64 [Q]: the sum over the counted rows of (max z - z_y) + log sum_c exp(z_c - max z);
 * correct, counted int32 [Q].  Thread t adds rows t, t + DVAE_LR_PREDICT_THREADS, ... in that order, the lanes of a wave by a
 * fixed shuffle tree, the waves in their order.  Every element is written.  1 <= T <= 2^31 - 1.                                 */
int dvae_lr_predict(const float* features, const double* shift, const double* scale, const int32_t* labels,
                    const int32_t* n_classes, long T, int D, int Q, const double* coef, float* prob, double* log_loss,
                    int32_t* correct, int32_t* counted, void* stream);

#ifdef __cplusplus
}
#endif
#endif
