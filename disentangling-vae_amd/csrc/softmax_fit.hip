// libdvae_lr_hip.so (include/dvae_lr_hip.h): the multinomial logistic regression behind the beta-VAE score, explicitness and InfoE
// fitted on the device -- a truncated Newton-CG iteration in fp64, one persistent workgroup per problem, the whole solve in one
// launch -- and the evaluation of the fits.
//
// k_lr_fit.  One workgroup per problem.  An EVALUATION at theta is a pass over the rows (thread t owns rows t, t + 512, ...: the
// logits of a row are formed 16 features at a time from registers and live, class-major, in the workspace; the softmax of a row is
// done by its thread, so the pass needs no barrier) and a sum over the rows (rows_sum: the (chunk, entry) partials, each added in
// row order by one thread, then the partials of an entry in chunk order).  A Hessian-vector product is the same two steps with
// r_ic = p_ic (u_ic - sum_c' p_ic' u_ic'), u = X v, in the second buffer.  Sums over the entries of a vector and over the rows'
// losses go through block_sum: the same bits in EVERY thread, so every branch of the solver is uniform.
// k_lr_predict.  One workgroup per problem walks the T rows; a thread keeps its row (fp32) in its own column of the LDS and forms
// the logits up to three times (arg-max, sum of exponentials, probabilities) instead of storing them.
#include <math.h>

#include "../../include/dvae_lr_hip.h"
#include "common.h"
#include "last_error.h"
#include "table_stats.h"

namespace dvae {

namespace {

#define LR_T DVAE_LR_THREADS
#define LR_WAVES (LR_T / 64)
#define LR_DT DVAE_LR_FEATURE_TILE
#define LR_PT DVAE_LR_PREDICT_THREADS
#define LR_PWAVES (LR_PT / 64)
#define LR_VECTORS 8                                             // theta, gradient, trial point, its gradient (the conjugate direction between trials), direction, residual, H v, 1 / diag H
#define LR_NQ 3                                                  // numbers of one block_sum

static_assert(LR_T % 64 == 0 && LR_T <= 1024 && LR_PT % 64 == 0, "whole waves");
static_assert(DVAE_LR_MAX_D % LR_DT == 0, "the feature tiles cover a row");
static_assert(4L * DVAE_LR_MAX_D * LR_PT + 16L * DVAE_LR_MAX_D + 1024 <= 64L * 1024, "k_lr_predict's static LDS");

struct Plan {                                                    // where problem q lives in the workspace (doubles) and in coef
  int C[DVAE_LR_MAX_PROBLEMS];
  int n_chunks[DVAE_LR_MAX_PROBLEMS];
  int chunk[DVAE_LR_MAX_PROBLEMS];
  long ws_at[DVAE_LR_MAX_PROBLEMS];
  long coef_at[DVAE_LR_MAX_PROBLEMS];
  long prob_at[DVAE_LR_MAX_PROBLEMS];                            // dvae_lr_predict: elements of prob before problem q
};

struct Sums {
  double q[LR_NQ];
};

// the sum of every thread's q, the same bits in every thread: the shuffle tree of a wave, then the waves in their order
__device__ __forceinline__ Sums block_sum(Sums v, double* __restrict__ scratch, int* n_pass) {
  double* buf = scratch + (*n_pass & 1) * (LR_WAVES * LR_NQ);
  ++*n_pass;
#pragma unroll
  for (int k = 0; k < LR_NQ; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v.q[k] += __shfl_down(v.q[k], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < LR_NQ; ++k) buf[(threadIdx.x >> 6) * LR_NQ + k] = v.q[k];
  }
  __syncthreads();
  Sums r;
#pragma unroll
  for (int k = 0; k < LR_NQ; ++k) {
    double a = buf[k];
#pragma unroll
    for (int wv = 1; wv < LR_WAVES; ++wv) a += buf[wv * LR_NQ + k];
    r.q[k] = a;
  }
  return r;
}

// the largest of every thread's v (>= 0), in every thread
__device__ __forceinline__ double block_max(double v, double* __restrict__ scratch, int* n_pass) {
  double* buf = scratch + (*n_pass & 1) * (LR_WAVES * LR_NQ);
  ++*n_pass;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  double a = buf[0];
#pragma unroll
  for (int wv = 1; wv < LR_WAVES; ++wv) a = fmax(a, buf[wv]);
  return a;
}

// feature d of a row: sh = (shift [MAX_D], scale [MAX_D]) in LDS
__device__ __forceinline__ double feature(float v, const double* __restrict__ sh, int d, bool scaled) {
  const double x = (double)v;
  return scaled ? (x - sh[d]) * sh[DVAE_LR_MAX_D + d] : x;
}

struct Rows {                                                    // what every pass over the rows of a problem reads
  const float* X;
  const double* sh;
  const int32_t* labels;
  int S, D, C, n_chunks, chunk;
  bool scaled;
};

// out[c, i] = b_c + sum_d W_cd x_id of row i at th = (W, b): LR_DT features at a time from registers, ascending d
__device__ __forceinline__ void row_logits(const Rows& r, int i, const double* __restrict__ th, double* __restrict__ out) {
  for (int d0 = 0; d0 < r.D; d0 += LR_DT) {
    double x[LR_DT];
#pragma unroll
    for (int j = 0; j < LR_DT; ++j) x[j] = d0 + j < r.D ? feature(r.X[(long)i * r.D + d0 + j], r.sh, d0 + j, r.scaled) : 0.;
    for (int c = 0; c < r.C; ++c) {
      const double* w = th + (long)c * r.D + d0;
      double acc = d0 == 0 ? th[(long)r.C * r.D + c] : out[(long)c * r.S + i];
#pragma unroll
      for (int j = 0; j < LR_DT; ++j) acc += (d0 + j < r.D ? w[j] : 0.) * x[j];
      out[(long)c * r.S + i] = acc;
    }
  }
}

// the pass of an evaluation: p[c, i] = softmax of row i at th; returns this thread's sum of the rows' losses
__device__ __forceinline__ double rows_softmax(const Rows& r, const double* __restrict__ th, double* __restrict__ p) {
  double loss = 0.;
  for (int i = threadIdx.x; i < r.S; i += LR_T) {
    row_logits(r, i, th, p);
    const int y = r.labels[i];
    double m = p[i], zy = 0.;
    for (int c = 0; c < r.C; ++c) {
      const double z = p[(long)c * r.S + i];
      m = fmax(m, z);
      if (c == y) zy = z;
    }
    double sum = 0.;
    for (int c = 0; c < r.C; ++c) {
      const double e = exp(p[(long)c * r.S + i] - m);
      p[(long)c * r.S + i] = e;
      sum += e;
    }
    for (int c = 0; c < r.C; ++c) p[(long)c * r.S + i] /= sum;
    loss += (m - zy) + log(sum);
  }
  return loss;
}

// the pass of a Hessian-vector product: u[c, i] = p_ic (u_ic - sum_c' p_ic' u_ic') with u = X v
__device__ __forceinline__ void rows_curvature(const Rows& r, const double* __restrict__ v, const double* __restrict__ p,
                                               double* __restrict__ u) {
  for (int i = threadIdx.x; i < r.S; i += LR_T) {
    row_logits(r, i, v, u);
    double s = 0.;
    for (int c = 0; c < r.C; ++c) s += p[(long)c * r.S + i] * u[(long)c * r.S + i];
    for (int c = 0; c < r.C; ++c) u[(long)c * r.S + i] = p[(long)c * r.S + i] * (u[(long)c * r.S + i] - s);
  }
}

// out = (1 / S) X1^T src + reg (pen_W, 0) in theta's layout, X1 = (X, 1).  SUM_RESIDUAL: src[c, i] - [labels[i] == c] takes src's
// place (the gradient); SUM_DIAGONAL: src (1 - src) takes src's place, x^2 takes x's and 1 takes pen's (the diagonal of H).
// The (chunk, entry) partials in row order, then the partials of an entry in chunk order.  Barriers inside: every thread calls.
enum { SUM_PLAIN = 0, SUM_RESIDUAL = 1, SUM_DIAGONAL = 2 };
__device__ __forceinline__ void rows_sum(const Rows& r, const double* __restrict__ src, int mode, const double* __restrict__ pen,
                                         double reg, double* __restrict__ part, double* __restrict__ out) {
  const int D1 = r.D + 1, P = r.C * D1;
  __syncthreads();                                               // src was written row by row by other threads
  for (int idx = threadIdx.x; idx < r.n_chunks * P; idx += LR_T) {
    const int k = idx / P, o = idx - k * P, c = o / D1, d = o - c * D1;
    const int i0 = k * r.chunk, i1 = lesser(r.S, i0 + r.chunk);
    const double* col = src + (long)c * r.S;
    double a = 0.;
    for (int i = i0; i < i1; ++i) {
      double rv = col[i];
      if (mode == SUM_RESIDUAL && r.labels[i] == c) rv -= 1.;
      if (mode == SUM_DIAGONAL) rv = rv * (1. - rv);
      double xv = d < r.D ? feature(r.X[(long)i * r.D + d], r.sh, d, r.scaled) : 1.;
      if (mode == SUM_DIAGONAL) xv = xv * xv;
      a += rv * xv;
    }
    part[idx] = a;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < P; o += LR_T) {
    double a = part[o];
    for (int k = 1; k < r.n_chunks; ++k) a += part[(long)k * P + o];
    const int c = o / D1, d = o - c * D1;
    const long at = d < r.D ? (long)c * r.D + d : (long)r.C * r.D + c;
    out[at] = a / (double)r.S + (d < r.D ? (mode == SUM_DIAGONAL ? reg : reg * pen[at]) : 0.);
  }
  __syncthreads();
}

struct Value {
  double f, gmax, gg;
};

// f and g at th (g into `g`, the probabilities into `p`)
__device__ __forceinline__ Value evaluate(const Rows& r, const double* __restrict__ th, double reg, double* __restrict__ p,
                                          double* __restrict__ part, double* __restrict__ g, double* __restrict__ scratch, int* n_pass) {
  Sums s = {};
  s.q[0] = rows_softmax(r, th, p);
  rows_sum(r, p, SUM_RESIDUAL, th, reg, part, g);
  const int P = r.C * (r.D + 1), PW = r.C * r.D;
  double gm = 0.;
  for (int o = threadIdx.x; o < P; o += LR_T) {
    const double gv = g[o];
    if (o < PW) s.q[1] += th[o] * th[o];
    s.q[2] += gv * gv;
    gm = fmax(gm, fabs(gv));
  }
  const Sums t = block_sum(s, scratch, n_pass);
  Value v;
  v.f = t.q[0] / (double)r.S + 0.5 * reg * t.q[1];
  v.gg = t.q[2];
  v.gmax = block_max(gm, scratch, n_pass);
  return v;
}

__global__ __launch_bounds__(LR_T) void k_lr_fit(const float* __restrict__ X, const double* __restrict__ shift,
                                                 const double* __restrict__ scale, const int32_t* __restrict__ labels, Plan plan, int S,
                                                 int D, double Creg, double tol, double* __restrict__ ws, double* __restrict__ coef,
                                                 double* __restrict__ report) {
  __shared__ double scratch[2 * LR_WAVES * LR_NQ];
  __shared__ double sh[2 * DVAE_LR_MAX_D];
  const int q = blockIdx.x, t = threadIdx.x;
  Rows r;
  r.X = X;
  r.sh = sh;
  r.labels = labels + (long)q * S;
  r.S = S;
  r.D = D;
  r.C = plan.C[q];
  r.n_chunks = plan.n_chunks[q];
  r.chunk = plan.chunk[q];
  r.scaled = shift != nullptr;
  if (r.scaled && t < D) {
    sh[t] = shift[t];
    sh[DVAE_LR_MAX_D + t] = scale[t];
  }
  const int P = r.C * (D + 1);
  double* p = ws + plan.ws_at[q];                                // [C, S] the probabilities at the point evaluated last
  double* u = p + (long)r.C * S;                                 // [C, S] the rows of a Hessian-vector product
  double* part = u + (long)r.C * S;                              // [n_chunks, P]
  double* vec = part + (long)r.n_chunks * P;
  double *th = vec, *g = vec + P, *th2 = vec + 2L * P, *g2 = vec + 3L * P, *dir = vec + 4L * P, *res = vec + 5L * P, *hp = vec + 6L * P,
         *minv = vec + 7L * P;
  double* cgp = g2;                                              // the conjugate direction: g2 is written only by a trial evaluation, after it
  for (int o = t; o < P; o += LR_T) th[o] = 0.;
  __syncthreads();                                               // sh and theta are read by every thread
  const double reg = 1. / (Creg * (double)S);
  int n_pass = 0;
  Value cur = evaluate(r, th, reg, p, part, g, scratch, &n_pass);
  double n_eval = 1.;
  int iters = -1;
  bool done = false;
  for (int it = 0; it <= DVAE_LR_MAX_ITERATIONS && !done; ++it) {
    if (cur.gmax <= tol) {
      iters = it;
      done = true;
    } else if (it < DVAE_LR_MAX_ITERATIONS) {
      // ---- conjugate gradients on H s = -g, preconditioned by the diagonal of H
      rows_sum(r, p, SUM_DIAGONAL, th, reg, part, minv);
      Sums sb = {};
      for (int o = t; o < P; o += LR_T) sb.q[0] += o >= r.C * D ? minv[o] : 0.;
      const double bias_diag = block_sum(sb, scratch, &n_pass).q[0] / (double)r.C;   // ONE number for the biases: the steps stay on sum b = 0
      Sums s0 = {};
      for (int o = t; o < P; o += LR_T) {
        const double dg = o >= r.C * D ? bias_diag : minv[o], mi = dg > 0. ? 1. / dg : 1.;
        minv[o] = mi;
        dir[o] = 0.;
        res[o] = -g[o];
        cgp[o] = -g[o] * mi;
        s0.q[0] += g[o] * g[o] * mi;
      }
      double rz = block_sum(s0, scratch, &n_pass).q[0];           // (its barrier: cgp is read by every thread from here on)
      const double gnorm = sqrt(cur.gg), cg_tol = fmin(0.5, sqrt(gnorm)) * gnorm;
      bool cg_done = false;
      for (int j = 0; j < DVAE_LR_MAX_CG && !cg_done; ++j) {
        rows_curvature(r, cgp, p, u);
        rows_sum(r, u, SUM_PLAIN, cgp, reg, part, hp);
        Sums s = {};
        for (int o = t; o < P; o += LR_T) s.q[0] += cgp[o] * hp[o];
        const double curv = block_sum(s, scratch, &n_pass).q[0];
        if (!(curv > 0.)) {                                      // no curvature along the direction (rounding only): keep what there is
          if (j == 0) {
            for (int o = t; o < P; o += LR_T) dir[o] = res[o] * minv[o];
          }
          cg_done = true;
        } else {
          const double alpha = rz / curv;
          Sums s2 = {};
          for (int o = t; o < P; o += LR_T) {
            dir[o] += alpha * cgp[o];
            const double rv = res[o] - alpha * hp[o];
            res[o] = rv;
            s2.q[0] += rv * rv;
            s2.q[1] += rv * rv * minv[o];
          }
          const Sums t2 = block_sum(s2, scratch, &n_pass);
          if (sqrt(t2.q[0]) <= cg_tol) {
            cg_done = true;
          } else {
            const double beta = t2.q[1] / rz;
            for (int o = t; o < P; o += LR_T) cgp[o] = res[o] * minv[o] + beta * cgp[o];
            rz = t2.q[1];
          }
        }
        __syncthreads();
      }
      Sums s = {};
      for (int o = t; o < P; o += LR_T) s.q[0] += g[o] * dir[o];
      const double slope = block_sum(s, scratch, &n_pass).q[0];
      // ---- the step
      double step = 1.;
      bool accepted = false;
      Value cand = cur;
      for (int hv = 0; hv <= DVAE_LR_MAX_HALVINGS && !accepted; ++hv) {
        for (int o = t; o < P; o += LR_T) th2[o] = th[o] + step * dir[o];
        __syncthreads();
        cand = evaluate(r, th2, reg, p, part, g2, scratch, &n_pass);
        n_eval += 1.;
        if (cand.f <= cur.f + 1e-4 * step * slope || (cand.f <= cur.f + 1e-12 * fabs(cur.f) && cand.gmax < cur.gmax)) {
          accepted = true;
        } else {
          step *= 0.5;
        }
      }
      if (accepted) {
        double* sw = th;
        th = th2;
        th2 = sw;
        sw = g;
        g = g2;
        g2 = sw;
        cgp = g2;
        cur = cand;
      } else {                                                   // nothing along the direction is acceptable: th and g stand, not converged
        done = true;
      }
    }
  }
  __syncthreads();
  for (int o = t; o < P; o += LR_T) coef[plan.coef_at[q] + o] = th[o];
  if (t == 0) {
    report[4 * q] = cur.f;
    report[4 * q + 1] = cur.gmax;
    report[4 * q + 2] = (double)iters;
    report[4 * q + 3] = n_eval;
  }
}

__global__ __launch_bounds__(LR_PT) void k_lr_predict(const float* __restrict__ X, const double* __restrict__ shift,
                                                      const double* __restrict__ scale, const int32_t* __restrict__ labels, Plan plan, long T,
                                                      int D, const double* __restrict__ coef, float* __restrict__ prob,
                                                      double* __restrict__ log_loss, int32_t* __restrict__ correct,
                                                      int32_t* __restrict__ counted) {
  __shared__ float xs[DVAE_LR_MAX_D * LR_PT];                    // feature d of this thread's row at [d * LR_PT + thread]
  __shared__ double sh[2 * DVAE_LR_MAX_D];
  __shared__ double part_loss[LR_PWAVES];
  __shared__ int part_n[2 * LR_PWAVES];
  const int q = blockIdx.x, t = threadIdx.x, C = plan.C[q];
  const bool scaled = shift != nullptr;
  if (scaled && t < D) {
    sh[t] = shift[t];
    sh[DVAE_LR_MAX_D + t] = scale[t];
  }
  __syncthreads();
  const double* W = coef + plan.coef_at[q];
  const double* b = W + (long)C * D;
  const int32_t* lab = labels + (long)q * T;
  float* out = prob ? prob + plan.prob_at[q] : nullptr;
  double loss = 0.;
  int n_ok = 0, n_counted = 0;
  for (long i = t; i < T; i += LR_PT) {
    for (int d = 0; d < D; ++d) xs[d * LR_PT + t] = X[i * D + d];
    const int y = lab[i];
    double m = 0., zy = 0.;
    int best = 0;
    for (int c = 0; c < C; ++c) {
      double z = b[c];
      for (int d = 0; d < D; ++d) z += W[(long)c * D + d] * feature(xs[d * LR_PT + t], sh, d, scaled);
      if (c == 0 || z > m) {                                     // ties: the lowest class stays
        m = z;
        best = c;
      }
      if (c == y) zy = z;
    }
    double sum = 0.;
    for (int c = 0; c < C; ++c) {
      double z = b[c];
      for (int d = 0; d < D; ++d) z += W[(long)c * D + d] * feature(xs[d * LR_PT + t], sh, d, scaled);
      sum += exp(z - m);
    }
    if (out) {
      for (int c = 0; c < C; ++c) {
        double z = b[c];
        for (int d = 0; d < D; ++d) z += W[(long)c * D + d] * feature(xs[d * LR_PT + t], sh, d, scaled);
        out[i * C + c] = (float)(exp(z - m) / sum);
      }
    }
    if (y >= 0) {
      loss += (m - zy) + log(sum);
      ++n_counted;
      n_ok += best == y ? 1 : 0;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    loss += __shfl_down(loss, off, 64);
    n_ok += __shfl_down(n_ok, off, 64);
    n_counted += __shfl_down(n_counted, off, 64);
  }
  if ((t & 63) == 0) {
    part_loss[t >> 6] = loss;
    part_n[t >> 6] = n_ok;
    part_n[LR_PWAVES + (t >> 6)] = n_counted;
  }
  __syncthreads();
  if (t == 0) {
    double a = part_loss[0];
    int ok = part_n[0], cnt = part_n[LR_PWAVES];
#pragma unroll
    for (int wv = 1; wv < LR_PWAVES; ++wv) {
      a += part_loss[wv];
      ok += part_n[wv];
      cnt += part_n[LR_PWAVES + wv];
    }
    log_loss[q] = a;
    correct[q] = ok;
    counted[q] = cnt;
  }
}

// the plan of Q problems on `rows` rows -> doubles of workspace, or -1
long make_plan(long rows, int D, const int32_t* n_classes, int Q, bool fit, Plan* plan) {
  if (!n_classes || Q < 1 || Q > DVAE_LR_MAX_PROBLEMS || D < 1 || D > DVAE_LR_MAX_D || rows < 1) return -1;
  if (fit && rows > DVAE_LR_MAX_ROWS) return -1;
  long at = 0, coef_at = 0, prob_at = 0;
  for (int q = 0; q < DVAE_LR_MAX_PROBLEMS; ++q) {
    const int C = q < Q ? n_classes[q] : 1;
    if (C < 1 || C > DVAE_LR_MAX_CLASSES) return -1;
    const long P = (long)C * (D + 1);
    long chunk = rows;
    const int n_chunks = fit ? chunks_of(rows, DVAE_LR_CHUNK_ROWS, LR_T / P >= 1 ? LR_T / P : 1, &chunk) : 1;
    plan->C[q] = C;
    plan->n_chunks[q] = n_chunks;
    plan->chunk[q] = (int)lesser(chunk, 2147483647L);
    plan->ws_at[q] = at;
    plan->coef_at[q] = coef_at;
    plan->prob_at[q] = prob_at;
    if (q < Q) {
      at += 2 * (long)C * rows + (long)n_chunks * P + LR_VECTORS * P;
      coef_at += P;
      prob_at += rows * C;
    }
  }
  return at;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_lr_version(void) { return DVAE_LR_VERSION; }
const char* dvae_lr_last_error(void) { return last_error(); }

long dvae_lr_ws_bytes(long S, int D, const int32_t* n_classes, int Q) {
  Plan plan;
  const long doubles = make_plan(S, D, n_classes, Q, true, &plan);
  return doubles < 0 ? -1 : 8 * doubles;
}

int dvae_lr_fit(const float* features, const double* shift, const double* scale, const int32_t* labels, const int32_t* n_classes,
                long S, int D, int Q, double C, double tolerance_grad, void* ws, double* coef, double* report, void* stream) {
  DVAE_CHECK_ARG(features && labels && n_classes && ws && coef && report);
  DVAE_CHECK_ARG((shift == nullptr) == (scale == nullptr));
  DVAE_CHECK_ARG(S >= 1 && S <= DVAE_LR_MAX_ROWS);
  DVAE_CHECK_ARG(D >= 1 && D <= DVAE_LR_MAX_D);
  DVAE_CHECK_ARG(Q >= 1 && Q <= DVAE_LR_MAX_PROBLEMS);
  DVAE_CHECK_ARG(C > 0. && C <= 1.7976931348623157e308);
  DVAE_CHECK_ARG(tolerance_grad >= 0. && tolerance_grad <= 1.7976931348623157e308);
  DVAE_CHECK_ARG(((uintptr_t)ws & 7) == 0);
  Plan plan;
  DVAE_CHECK_ARG(make_plan(S, D, n_classes, Q, true, &plan) >= 0);
  hipLaunchKernelGGL(k_lr_fit, dim3(Q), dim3(LR_T), 0, (hipStream_t)stream, features, shift, scale, labels, plan, (int)S, D, C,
                     tolerance_grad, (double*)ws, coef, report);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_lr_predict(const float* features, const double* shift, const double* scale, const int32_t* labels,
                    const int32_t* n_classes, long T, int D, int Q, const double* coef, float* prob, double* log_loss,
                    int32_t* correct, int32_t* counted, void* stream) {
  DVAE_CHECK_ARG(features && labels && n_classes && coef && log_loss && correct && counted);
  DVAE_CHECK_ARG((shift == nullptr) == (scale == nullptr));
  DVAE_CHECK_ARG(T >= 1 && T <= 2147483647L);
  DVAE_CHECK_ARG(D >= 1 && D <= DVAE_LR_MAX_D);
  DVAE_CHECK_ARG(Q >= 1 && Q <= DVAE_LR_MAX_PROBLEMS);
  Plan plan;
  DVAE_CHECK_ARG(make_plan(T, D, n_classes, Q, false, &plan) >= 0);
  hipLaunchKernelGGL(k_lr_predict, dim3(Q), dim3(LR_PT), 0, (hipStream_t)stream, features, shift, scale, labels, plan, T, D, coef, prob,
                     log_loss, correct, counted);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
