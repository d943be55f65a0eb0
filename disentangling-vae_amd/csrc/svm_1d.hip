// libdvae_sap_hip.so (include/dvae_sap_hip.h): the discrete-factor SAP score -- every one-feature, one-vs-rest squared-hinge SVM of
// disentanglement_lib's sap_score.py (LinearSVC(C = 0.01, class_weight = "balanced") on ONE latent) fitted on the device.
//
// k_sap_fit.  One workgroup per (problem, latent).  It gathers x_i = table[rows[i], d] (fp32) and the side of every row (one byte:
// the row carries the problem's class) ONCE into LDS, counts the positives for the balanced class weight, and runs Newton's
// method on the active set there (the header's recursion).  A PASS over the column at a point (w, b) gives the five weighted sums
// over the active rows, the objective, and the number of rows whose activity differs from that at the current point; thread t
// adds rows t, t + 256, ... in that order, the 64 lanes of a wave are combined by a fixed shuffle tree and the four waves in
// their order -- by EVERY thread, so all of them hold the same bits and every branch below is uniform.  The scratch of the wave
// partials is double-buffered by the parity of the pass: one barrier per pass.  The simple row walk, not a sorted column with
// prefix sums: DESIGN.md says what it costs.
// k_sap_accuracy.  One workgroup per (factor, latent): the coefficients of the factor's problems in LDS, every thread walks its
// rows, forms the decision values WITHOUT a fused multiply-add and picks the class; the counts are combined as above.
#include "../../include/dvae_sap_hip.h"
#include "common.h"
#include "last_error.h"

// the decision value is fl(fl(w x) + b), and the numpy restatement of the Newton recursion rounds every product too: nothing in
// this file may be contracted into a fused multiply-add (hipcc contracts by default)
#pragma clang fp contract(off)

namespace dvae {

namespace {

#define SAP_T DVAE_SAP_THREADS
#define SAP_WAVES (SAP_T / 64)
#define SAP_Q 7                                                  // numbers of one pass
#define SAP_SCRATCH (2 * SAP_WAVES * SAP_Q)                      // doubles at the head of the LDS

static_assert(SAP_T % 64 == 0 && SAP_T <= 1024, "whole waves");
static_assert(DVAE_SAP_MAX_ROWS >= 10240, "DCI's row count runs from LDS");
static_assert(8L * SAP_SCRATCH + 5L * DVAE_SAP_MAX_ROWS + 16 <= 160L * 1024, "the LDS of one CU");
static_assert(DVAE_SAP_MAX_CLASSES * 16 <= 64 * 1024, "the coefficients of one factor in LDS");

struct Classes {
  int c[DVAE_SAP_MAX_FACTORS];                                   // classes present per factor (1 beyond K)
};

__host__ __device__ __forceinline__ int problems_of(int C) { return C >= 3 ? C : C == 2 ? 1 : 0; }

struct Pass {
  double q[SAP_Q];                                               // S1, Sx, Sxx, Rx, R1, objective, rows whose activity changed
};

// the sum of every thread's q, the same bits in every thread: the shuffle tree of a wave, then the waves in their order
__device__ __forceinline__ Pass block_sum(Pass v, double* __restrict__ scratch, int* n_pass) {
  double* buf = scratch + (*n_pass & 1) * (SAP_WAVES * SAP_Q);
  ++*n_pass;
#pragma unroll
  for (int k = 0; k < SAP_Q; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v.q[k] += __shfl_down(v.q[k], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < SAP_Q; ++k) buf[(threadIdx.x >> 6) * SAP_Q + k] = v.q[k];
  }
  __syncthreads();
  Pass r;
#pragma unroll
  for (int k = 0; k < SAP_Q; ++k) {
    double a = buf[k];
#pragma unroll
    for (int wv = 1; wv < SAP_WAVES; ++wv) a += buf[wv * SAP_Q + k];
    r.q[k] = a;
  }
  return r;
}

// one pass at (w, b); compare: count the rows whose activity differs from that at (w0, b0)
__device__ __forceinline__ Pass column_pass(const float* __restrict__ xs, const uint8_t* __restrict__ side, int S, double cp, double cn,
                                            double w, double b, double w0, double b0, bool compare, double* __restrict__ scratch,
                                            int* n_pass) {
  Pass a = {};
  for (int i = threadIdx.x; i < S; i += SAP_T) {
    const double x = (double)xs[i];
    const bool pos = side[i] != 0;
    const double s = pos ? 1. : -1., c = pos ? cp : cn;
    const double m = s * (w * x + b);
    const bool active = m < 1.;
    if (compare && active != (s * (w0 * x + b0) < 1.)) a.q[6] += 1.;
    if (active) {
      const double cx = c * x, cs = c * s, r = 1. - m;
      a.q[0] += c;
      a.q[1] += cx;
      a.q[2] += cx * x;
      a.q[3] += cs * x;
      a.q[4] += cs;
      a.q[5] += c * r * r;
    }
  }
  Pass t = block_sum(a, scratch, n_pass);
  t.q[5] += 0.5 * (w * w + b * b);
  return t;
}

__global__ __launch_bounds__(SAP_T) void k_sap_fit(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                   const int32_t* __restrict__ labels, Classes cls, int D, int K, int S, int P, double C,
                                                   double* __restrict__ coef, int32_t* __restrict__ iterations) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* scratch = lds;                                         // [2][waves][SAP_Q]
  float* xs = (float*)(lds + SAP_SCRATCH);                       // [S]
  uint8_t* side = (uint8_t*)(xs + S);                            // [S]
  const int d = blockIdx.y;
  int p = blockIdx.x, j = 0, k = 0, Cj = 1;
  bool found = false;
#pragma unroll
  for (int f = 0; f < DVAE_SAP_MAX_FACTORS; ++f) {               // the problem's factor and class (the same in every thread)
    const int np = f < K ? problems_of(cls.c[f]) : 0;
    if (!found && p < np) {
      found = true;
      j = f;
      Cj = cls.c[f];
      k = Cj == 2 ? 1 : p;
    }
    if (!found) p -= np;
  }
  if (!found) return;                                            // (the grid is P wide: not reached)
  int n_pass = 0;
  Pass cnt = {};
  for (int i = threadIdx.x; i < S; i += SAP_T) {
    const bool pos = labels[(long)j * S + i] == k;
    xs[i] = table[rows[i] * D + d];
    side[i] = pos ? 1 : 0;
    if (pos) cnt.q[0] += 1.;
  }
  __syncthreads();                                               // the column is read by other threads from here on
  const double n_pos = block_sum(cnt, scratch, &n_pass).q[0], n_neg = (double)S - n_pos;
  const long out = (long)d * P + blockIdx.x;
  if (!(n_pos >= 1.) || (Cj == 2 && !(n_neg >= 1.))) {           // a class no training row carries: the caller's labels are wrong
    if (threadIdx.x == 0) {
      coef[2 * out] = 0.;
      coef[2 * out + 1] = 0.;
      iterations[out] = -1;
    }
    return;
  }
  // class_weight = "balanced": S / (classes present * count); liblinear weighs the positives of a one-vs-rest problem only
  const double cp = C * ((double)S / ((double)Cj * n_pos));
  const double cn = Cj == 2 ? C * ((double)S / ((double)Cj * n_neg)) : C;
  double w = 0., b = 0.;
  Pass cur = column_pass(xs, side, S, cp, cn, w, b, 0., 0., false, scratch, &n_pass);
  int iters = -1;
  bool done = false;
  for (int it = 1; it <= DVAE_SAP_MAX_ITERATIONS && !done; ++it) {
    const double a = 1. + 2. * cur.q[2], h = 2. * cur.q[1], e = 1. + 2. * cur.q[0], rx = 2. * cur.q[3], r1 = 2. * cur.q[4];
    const double det = a * e - h * h;
    const double wf = (e * rx - h * r1) / det, bf = (a * r1 - h * rx) / det;      // the minimiser of the current piece
    double t = 1., cw = wf, cb = bf;
    Pass cand = cur;
    bool accepted = false;
    for (int hv = 0; hv <= DVAE_SAP_MAX_HALVINGS && !accepted && !done; ++hv) {
      cw = hv == 0 ? wf : w + t * (wf - w);
      cb = hv == 0 ? bf : b + t * (bf - b);
      cand = column_pass(xs, side, S, cp, cn, cw, cb, w, b, true, scratch, &n_pass);
      if (hv == 0 && cand.q[6] == 0.) {                          // the full step keeps the active set: the exact minimiser
        w = cw;
        b = cb;
        iters = it;
        done = true;
      } else if (cand.q[5] < cur.q[5]) {
        accepted = true;
      } else {
        t *= 0.5;
      }
    }
    if (!done) {
      if (accepted) {
        w = cw;
        b = cb;
        cur = cand;
      } else {                                                   // nothing along the step lowers the objective: the minimiser to rounding
                                                                 // (a row exactly ON the hinge at the optimum: the two pieces' minimisers are one
                                                                 // point in exact arithmetic and two in fp64, and the full step hops between them)
        iters = it;
        done = true;
      }
    }
  }
  if (threadIdx.x == 0) {
    coef[2 * out] = w;
    coef[2 * out + 1] = b;
    iterations[out] = iters;
  }
}

__device__ __forceinline__ double decision(double w, double x, double b) {
  const double prod = w * x;                                     // rounded: contraction is off in this file
  return prod + b;
}

__global__ __launch_bounds__(SAP_T) void k_sap_accuracy(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                        const int32_t* __restrict__ labels, Classes cls, int D, int K, long T, int P,
                                                        const double* __restrict__ coef, int32_t* __restrict__ correct,
                                                        int32_t* __restrict__ predicted) {
  __shared__ double wb[2 * DVAE_SAP_MAX_CLASSES];
  __shared__ int part[SAP_WAVES];
  const int j = blockIdx.x, d = blockIdx.y;
  int p0 = 0;
#pragma unroll
  for (int f = 0; f < DVAE_SAP_MAX_FACTORS; ++f)
    if (f < j) p0 += problems_of(cls.c[f]);
  const int Cj = cls.c[j], np = problems_of(Cj);
  for (int i = threadIdx.x; i < 2 * np; i += SAP_T) wb[i] = coef[2 * ((long)d * P + p0) + i];
  __syncthreads();
  int n = 0;
  for (long i = threadIdx.x; i < T; i += SAP_T) {
    const double x = (double)table[rows[i] * D + d];
    int pred = 0;
    if (Cj >= 3) {
      double best = decision(wb[0], x, wb[1]);
      for (int k = 1; k < Cj; ++k) {
        const double v = decision(wb[2 * k], x, wb[2 * k + 1]);
        if (v > best) {                                          // ties: the lowest class stays
          best = v;
          pred = k;
        }
      }
    } else if (Cj == 2) {
      pred = decision(wb[0], x, wb[1]) > 0. ? 1 : 0;
    }
    if (predicted) predicted[((long)d * K + j) * T + i] = pred;
    n += pred == labels[(long)j * T + i] ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int a = part[0];
#pragma unroll
    for (int wv = 1; wv < SAP_WAVES; ++wv) a += part[wv];
    correct[(long)d * K + j] = a;
  }
}

// the classes of the K factors -> P, or -1
long load_classes(const int32_t* n_classes, int K, Classes* cls) {
  if (!n_classes || K < 1 || K > DVAE_SAP_MAX_FACTORS) return -1;
  long P = 0;
  for (int f = 0; f < DVAE_SAP_MAX_FACTORS; ++f) {
    cls->c[f] = f < K ? n_classes[f] : 1;
    if (cls->c[f] < 1 || cls->c[f] > DVAE_SAP_MAX_CLASSES) return -1;
    P += problems_of(cls->c[f]);
  }
  return P;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_sap_version(void) { return DVAE_SAP_VERSION; }
const char* dvae_sap_last_error(void) { return last_error(); }

long dvae_sap_problems(const int32_t* n_classes, int K) {
  Classes cls;
  return load_classes(n_classes, K, &cls);
}

int dvae_sap_fit(const float* table, const int64_t* rows, const int32_t* labels, const int32_t* n_classes, long N, int D, int K,
                 long S, double C, double* coef, int32_t* iterations, void* stream) {
  DVAE_CHECK_ARG(table && rows && labels && n_classes);
  DVAE_CHECK_ARG(N >= 1 && N <= 2147483647L);
  DVAE_CHECK_ARG(D >= 1 && D <= DVAE_SAP_MAX_D);
  DVAE_CHECK_ARG(K >= 1 && K <= DVAE_SAP_MAX_FACTORS);
  DVAE_CHECK_ARG(S >= 1 && S <= DVAE_SAP_MAX_ROWS);
  DVAE_CHECK_ARG(C > 0. && C <= 1.7976931348623157e308);
  Classes cls;
  const long P = load_classes(n_classes, K, &cls);
  DVAE_CHECK_ARG(P >= 0);
  if (P == 0) return 0;                                          // every factor holds one class: no problem, nothing to write
  DVAE_CHECK_ARG(coef && iterations);
  const size_t lds = 8 * (size_t)SAP_SCRATCH + 5 * (size_t)S;
  static DeviceOnce attr;                                        // above 64 KiB of dynamic LDS (13 018 rows or more) the launch needs this
  if (attr.first() && hipFuncSetAttribute((const void*)k_sap_fit, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          8 * SAP_SCRATCH + 5 * DVAE_SAP_MAX_ROWS) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s:%d: the device refuses %d bytes of LDS per workgroup", __FILE__, __LINE__, 8 * SAP_SCRATCH + 5 * DVAE_SAP_MAX_ROWS);
    return -2;
  }
  hipLaunchKernelGGL(k_sap_fit, dim3((unsigned)P, D), dim3(SAP_T), lds, (hipStream_t)stream, table, rows, labels, cls, D, K, (int)S, (int)P, C,
                     coef, iterations);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_sap_accuracy(const float* table, const int64_t* rows, const int32_t* labels, const int32_t* n_classes, long N, int D,
                      int K, long T, const double* coef, int32_t* correct, int32_t* predicted, void* stream) {
  DVAE_CHECK_ARG(table && rows && labels && n_classes && correct);
  DVAE_CHECK_ARG(N >= 1 && N <= 2147483647L);
  DVAE_CHECK_ARG(D >= 1 && D <= DVAE_SAP_MAX_D);
  DVAE_CHECK_ARG(K >= 1 && K <= DVAE_SAP_MAX_FACTORS);
  DVAE_CHECK_ARG(T >= 1 && T <= 2147483647L);
  Classes cls;
  const long P = load_classes(n_classes, K, &cls);
  DVAE_CHECK_ARG(P >= 0);
  DVAE_CHECK_ARG(coef || P == 0);
  hipLaunchKernelGGL(k_sap_accuracy, dim3(K, D), dim3(SAP_T), 0, (hipStream_t)stream, table, rows, labels, cls, D, K, T, (int)P, coef, correct,
                     predicted);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
