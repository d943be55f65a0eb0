// libdvae_dci_hip.so (include/dvae_dci_hip.h): gradient-boosted depth-3 regression trees -- scikit-learn's
// GradientBoostingClassifier with default arguments, restated -- on S selected rows of an fp32 [N, D] table, for the DCI scores.
// The header states the model and the summation order; here is how a stage becomes DVAE_DCI_LAUNCHES_PER_STAGE launches, all
// T trees of the stage (and all D features) in one grid each:
//   k_dci_residual   a thread per row: p = softmax(raw_s) once, r[k][s] = y - p_k for every tree k;
//   k_dci_split<-1>  a workgroup per tree: every row to node 0, the root's (n, sum r, sum r^2, sum h);
//   k_dci_search     a workgroup per (feature, tree), levels 0, 1, 2: the column in sorted order is gathered ONCE into LDS
//                    (residual, value, open node of the level -- DVAE_DCI_ROW_LDS_BYTES a row, element j of thread t at
//                    j * 1024 + t: no bank conflicts); thread t owns positions [t c, (t + 1) c).  The running (count, sum r,
//                    last value) of each of the <= 4 open nodes is a segmented scan over rows that are NOT contiguous per node:
//                    chunk partials per thread, an in-workgroup scan of them (wave shuffles at doubling distances, then the
//                    waves before in order), and a second walk of the chunk out of LDS that starts from the prefix and
//                    evaluates the gain at every boundary between distinct values.  The best (gain, lo, hi) per node is reduced
//                    over the threads -- ties to the lower thread, i.e. the lower position -- and stored per (tree, node, feature);
//   k_dci_split<L>   a workgroup per tree: the arg-max over the features of each node of level L (ties to the lower feature),
//                    the node byte of every row of a split node moves to the child, and the children's statistics are added
//                    in the fixed order of the header.  k_dci_split<2> also ends the stage for its tree: leaf values, the
//                    raw-score update of its column of `raw`, the tree's importances.
// After the last stage k_dci_importance adds the per-tree importances in the order of the trees.  A node's statistics are
// computed once, by its tree's workgroup, and every feature's search reads those: the leaf test and the totals of the gain do not
// depend on the feature.  Node bytes hold heap indices; rows of a leaf above depth 3 keep its index and are skipped by the
// levels below.  Every loop bound is a function of the arguments.
#include <math.h>

#include "../../include/dvae_dci_hip.h"
#include "common.h"
#include "last_error.h"

namespace dvae {

namespace {

#define DCI_T DVAE_DCI_THREADS
#define DCI_WAVES (DCI_T / 64)
#define DCI_NODES DVAE_DCI_NODES
#define DCI_STATS DVAE_DCI_NODE_STATS
#define DCI_OPEN 4                                             // open nodes of a level: 1, 2, 4
#define DCI_WS_STATS 5                                         // n, sum r, sum r^2, sum h, open
#define DCI_LDS_MAX (DVAE_DCI_ROW_LDS_BYTES * DVAE_DCI_MAX_ROWS)
#define DCI_NO_NODE 255

static_assert(DVAE_DCI_MAX_ROWS % DCI_T == 0, "every thread owns the same number of positions");
static_assert(DVAE_DCI_ROW_LDS_BYTES == sizeof(double) + sizeof(float) + 1, "residual, value, node");
static_assert(DCI_LDS_MAX + DVAE_DCI_LDS_SCRATCH <= 160 * 1024, "a column and the scan scratch within the LDS of a compute unit");
static_assert(DVAE_DCI_MAX_D <= DCI_T && DVAE_DCI_MAX_CLASSES <= DCI_T, "a thread per feature / class");
static_assert(DCI_NODES == 15 && DCI_STATS == 5, "depth 3");

struct DciWs {                                                 // the workspace, 8-byte aligned
  double* r;                                                   // [T, S] residuals of the stage
  double* stats;                                               // [T, 15, DCI_WS_STATS]
  double* gain;                                                // [T, DCI_OPEN, D] best gain of a (tree, node, feature), -1: none
  float* lohi;                                                 // [T, DCI_OPEN, D, 2] the values it lies between
  double* imp;                                                 // [n_stages, T, D] per-tree importances
  int32_t* split;                                              // [n_stages, T]: the root split
  uint8_t* node;                                               // [T, S] heap index of the node a row is in
};
__host__ __device__ __forceinline__ DciWs dci_ws(float* ws, int D, int S, int T, int n_stages) {
  DciWs w;
  w.r = (double*)ws;
  w.stats = w.r + (long)T * S;
  w.gain = w.stats + (long)T * DCI_NODES * DCI_WS_STATS;
  w.imp = w.gain + (long)T * DCI_OPEN * D;
  w.lohi = (float*)(w.imp + (long)n_stages * T * D);
  w.split = (int32_t*)(w.lohi + (long)T * DCI_OPEN * D * 2);
  w.node = (uint8_t*)(w.split + (long)n_stages * T);
  return w;
}
size_t dci_ws_floats(int D, int S, int T, int n_stages) {
  const long doubles = (long)T * S + (long)T * DCI_NODES * DCI_WS_STATS + (long)T * DCI_OPEN * D + (long)n_stages * T * D;
  return (size_t)(2 * doubles + (long)T * DCI_OPEN * D * 2 + (long)n_stages * T + ((long)T * S + 3) / 4);
}

__host__ __device__ __forceinline__ int trees_of(int C) { return C <= 2 ? 1 : C; }
__device__ __forceinline__ double mse_of(double n, double sr, double srr) {
  const double m = sr / n;
  return srr / n - m * m;
}
// y of row s in tree k: two classes share one tree whose target is the label itself
__device__ __forceinline__ double target_of(int label, int k, int C) { return C == 2 ? (double)label : (label == k ? 1. : 0.); }

// sum over the 64 lanes of a wave, in lane 0: pairwise at distances 32 ... 1
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ---- prior ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DCI_T) void k_dci_prior(const int32_t* __restrict__ labels, int S, int C, double* __restrict__ prior) {
  __shared__ int cnt[DCI_T];
  __shared__ double lg[DCI_T];
  const int t = threadIdx.x;
  cnt[t] = 0;
  __syncthreads();
  for (int s = t; s < S; s += DCI_T) {                                   // integer counts: any order gives the same
    const unsigned label = (unsigned)labels[s];
    if (label < (unsigned)C) atomicAdd(&cnt[label], 1);
  }
  __syncthreads();
  const double e = 1.1920928955078125e-07;                               // 2^-23
  double q = (double)cnt[t < C ? t : 0] / (double)S;
  q = q < e ? e : (q > 1. - e ? 1. - e : q);
  if (C <= 2) {                                                          // the same in every thread
    if (t == 1) prior[0] = C == 2 ? log(q / (1. - q)) : 0.;
    return;
  }
  lg[t] = log(q);
  __syncthreads();
  if (t >= C) return;
  double sum = 0.;
  for (int k = 0; k < C; ++k) sum += lg[k];
  prior[t] = log(q / exp(sum / (double)C));
}

__global__ __launch_bounds__(DCI_T) void k_dci_fill_raw(const double* __restrict__ prior, int S, int T, double* __restrict__ raw) {
  const long i = blockIdx.x * (long)DCI_T + threadIdx.x;
  if (i < (long)S * T) raw[i] = prior[i % T];
}

// ---- residuals of a stage --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DCI_T) void k_dci_residual(const int32_t* __restrict__ labels, const double* __restrict__ raw, int S,
                                                        int C, int T, double* __restrict__ r) {
  const int s = blockIdx.x * DCI_T + threadIdx.x;
  if (s >= S) return;
  const int label = labels[s];
  const double* row = raw + (long)s * T;
  if (C == 2) {
    r[s] = (double)label - 1. / (1. + exp(-row[0]));
    return;
  }
  double top = row[0];
  for (int k = 1; k < T; ++k) top = row[k] > top ? row[k] : top;
  double sum = 0.;
  for (int k = 0; k < T; ++k) sum += exp(row[k] - top);
  for (int k = 0; k < T; ++k) r[(long)k * S + s] = target_of(label, k, C) - exp(row[k] - top) / sum;
}

// ---- split search of one (feature, tree) at one level ----------------------------------------------------------------------------
struct Run {                                                   // rows of one open node seen so far along the sorted column
  int cnt;
  double sum;
  float last;
};
__device__ __forceinline__ Run joined(const Run& a, const Run& b) {      // a lies before b
  Run c;
  c.cnt = a.cnt + b.cnt;
  c.sum = a.sum + b.sum;
  c.last = b.cnt > 0 ? b.last : a.last;
  return c;
}

__global__ __launch_bounds__(DCI_T) void k_dci_search(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                      const int32_t* __restrict__ order, int D, int S, int chunk, int level, int T,
                                                      int n_stages, float* ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dci_lds[];
  __shared__ int w_cnt[DCI_WAVES][DCI_OPEN];
  __shared__ double w_sum[DCI_WAVES][DCI_OPEN];
  __shared__ float w_last[DCI_WAVES][DCI_OPEN];
  __shared__ double w_gain[DCI_WAVES][DCI_OPEN];
  __shared__ float w_lo[DCI_WAVES][DCI_OPEN], w_hi[DCI_WAVES][DCI_OPEN];
  double* l_r = (double*)dci_lds;                              // [chunk, DCI_T]
  float* l_x = (float*)(l_r + (long)chunk * DCI_T);
  uint8_t* l_n = (uint8_t*)(l_x + (long)chunk * DCI_T);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, d = blockIdx.x, tree = blockIdx.y;
  const DciWs w = dci_ws(ws, D, S, T, n_stages);
  const int base = (1 << level) - 1, nopen = 1 << level;
  double tot_n[DCI_OPEN], tot_s[DCI_OPEN];
  unsigned open = 0u;
#pragma unroll
  for (int q = 0; q < DCI_OPEN; ++q) {
    tot_n[q] = tot_s[q] = 0.;
    if (q < nopen) {
      const double* st = w.stats + ((long)tree * DCI_NODES + base + q) * DCI_WS_STATS;
      tot_n[q] = st[0];
      tot_s[q] = st[1];
      if (st[4] != 0.) open |= 1u << q;
    }
  }
  const long rec = (long)tree * DCI_OPEN * D + d;                        // node q: + q * D
  if (open == 0u) {                                            // the same in every thread: no node of this level is open
    if (t < DCI_OPEN) w.gain[rec + (long)t * D] = -1.;
    return;
  }
  // walk 1: gather the chunk into LDS -- the loads of a position do not wait for its node byte and four positions are in flight --
  // then the partials of the chunk out of LDS (own elements: no barrier)
  const int i0 = t * chunk;
#pragma unroll 4
  for (int j = 0; j < chunk; ++j) {
    const int i = i0 + j;
    int q = DCI_NO_NODE;
    double rr = 0.;
    float x = 0.f;
    if (i < S) {
      const int s = order[(long)d * S + i];
      const int at = (int)w.node[(long)tree * S + s] - base;
      rr = w.r[(long)tree * S + s];
      x = table[(rows ? (long)rows[s] : (long)s) * D + d];
      if (at >= 0 && at < nopen && ((open >> at) & 1u)) q = at;
    }
    l_r[j * DCI_T + t] = rr;
    l_x[j * DCI_T + t] = x;
    l_n[j * DCI_T + t] = (uint8_t)q;
  }
  Run run[DCI_OPEN];
#pragma unroll
  for (int q = 0; q < DCI_OPEN; ++q) run[q].cnt = 0, run[q].sum = 0., run[q].last = 0.f;
  for (int j = 0; j < chunk; ++j) {
    const int q = l_n[j * DCI_T + t];
    const double rr = l_r[j * DCI_T + t];
    const float x = l_x[j * DCI_T + t];
#pragma unroll
    for (int k = 0; k < DCI_OPEN; ++k)
      if (q == k) run[k].cnt += 1, run[k].sum += rr, run[k].last = x;
  }
  // the prefix of the threads before this one: inclusive scan within the wave, shifted by one lane, then the waves before
#pragma unroll
  for (int q = 0; q < DCI_OPEN; ++q) {
    Run inc = run[q];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      Run before;
      before.cnt = __shfl_up(inc.cnt, o, 64);
      before.sum = __shfl_up(inc.sum, o, 64);
      before.last = __shfl_up(inc.last, o, 64);
      if (lane >= o) inc = joined(before, inc);
    }
    if (lane == 63) w_cnt[wv][q] = inc.cnt, w_sum[wv][q] = inc.sum, w_last[wv][q] = inc.last;
    Run exc;
    exc.cnt = __shfl_up(inc.cnt, 1, 64);
    exc.sum = __shfl_up(inc.sum, 1, 64);
    exc.last = __shfl_up(inc.last, 1, 64);
    if (lane == 0) exc.cnt = 0, exc.sum = 0., exc.last = 0.f;
    run[q] = exc;
  }
  __syncthreads();                                             // the wave totals, and the chunk in LDS (own elements only)
#pragma unroll
  for (int q = 0; q < DCI_OPEN; ++q) {
    Run head;
    head.cnt = 0, head.sum = 0., head.last = 0.f;
#pragma unroll
    for (int i = 0; i < DCI_WAVES - 1; ++i)
      if (i < wv) {
        Run one;
        one.cnt = w_cnt[i][q], one.sum = w_sum[i][q], one.last = w_last[i][q];
        head = joined(head, one);
      }
    run[q] = joined(head, run[q]);
  }
  // walk 2: the gain at every boundary between distinct values of a node
  double best[DCI_OPEN];
  float lo[DCI_OPEN], hi[DCI_OPEN];
#pragma unroll
  for (int q = 0; q < DCI_OPEN; ++q) best[q] = -1., lo[q] = hi[q] = 0.f;
  for (int j = 0; j < chunk; ++j) {
    const int q = l_n[j * DCI_T + t];
    if (q == DCI_NO_NODE) continue;
    const double rr = l_r[j * DCI_T + t];
    const float x = l_x[j * DCI_T + t];
#pragma unroll
    for (int k = 0; k < DCI_OPEN; ++k)
      if (q == k) {
        if (run[k].cnt > 0 && x > __fadd_rn(run[k].last, 1e-7f)) {
          const double nl = (double)run[k].cnt, sl = run[k].sum, nr = tot_n[k] - nl, sr = tot_s[k] - sl;
          const double diff = nr * sl - nl * sr;
          const double gain = diff * diff / (nl * nr);
          if (gain > best[k]) best[k] = gain, lo[k] = run[k].last, hi[k] = x;
        }
        run[k].cnt += 1, run[k].sum += rr, run[k].last = x;
      }
  }
  // the best of the workgroup per node: the larger gain, at equal gains the lower thread (its positions come first)
#pragma unroll
  for (int q = 0; q < DCI_OPEN; ++q) {
    double g = best[q];
    float a = lo[q], b = hi[q];
    int who = lane;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double g2 = __shfl_xor(g, o, 64);
      const float a2 = __shfl_xor(a, o, 64), b2 = __shfl_xor(b, o, 64);
      const int who2 = __shfl_xor(who, o, 64);
      if (g2 > g || (g2 == g && who2 < who)) g = g2, a = a2, b = b2, who = who2;
    }
    if (lane == 0) w_gain[wv][q] = g, w_lo[wv][q] = a, w_hi[wv][q] = b;
  }
  __syncthreads();
  if (t < DCI_OPEN) {
    double g = w_gain[0][t];
    float a = w_lo[0][t], b = w_hi[0][t];
#pragma unroll
    for (int i = 1; i < DCI_WAVES; ++i)
      if (w_gain[i][t] > g) g = w_gain[i][t], a = w_lo[i][t], b = w_hi[i][t];
    w.gain[rec + (long)t * D] = g;
    w.lohi[2 * (rec + (long)t * D)] = a;
    w.lohi[2 * (rec + (long)t * D) + 1] = b;
  }
}

// ---- split the nodes of level L (L = -1: make the root), the statistics of their children ---------------------------------------
template <int L>
__global__ __launch_bounds__(DCI_T) void k_dci_split(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                     const int32_t* __restrict__ labels, int D, int S, int chunk, int C, int T,
                                                     int n_stages, int stage, double learning_rate, float* ws,
                                                     double* __restrict__ raw, int32_t* __restrict__ tree_feature,
                                                     double* __restrict__ tree_stats) {
  constexpr int NP = L >= 0 ? (1 << L) : 1;                    // parents
  constexpr int PBASE = L >= 0 ? (1 << L) - 1 : 0;
  constexpr int NC = 1 << (L + 1);                             // children
  constexpr int CBASE = NC - 1;
  __shared__ int s_feat[DCI_NODES];
  __shared__ double s_thr[DCI_OPEN];
  __shared__ double s_val[DCI_NODES];
  __shared__ double s_st[DCI_NODES][4];
  __shared__ double s_part[NC][4][DCI_WAVES];
  const int t = threadIdx.x, tree = blockIdx.x;
  const DciWs w = dci_ws(ws, D, S, T, n_stages);
  double* stats = w.stats + (long)tree * DCI_NODES * DCI_WS_STATS;
  int32_t* feat_out = tree_feature + ((long)stage * T + tree) * DCI_NODES;
  double* stat_out = tree_stats + ((long)stage * T + tree) * DCI_NODES * DCI_STATS;
  if (L >= 0 && t < NP) {                                      // the arg-max over the features: the lowest feature among equals
    const int h = PBASE + t;
    int f = -1;
    double g = -1., thr = 0.;
    float a = 0.f, b = 0.f;
    if (stats[h * DCI_WS_STATS + 4] != 0.) {
      const long rec = ((long)tree * DCI_OPEN + t) * D;
      for (int d = 0; d < D; ++d)
        if (w.gain[rec + d] > g) g = w.gain[rec + d], f = d, a = w.lohi[2 * (rec + d)], b = w.lohi[2 * (rec + d) + 1];
    }
    if (f >= 0) {
      thr = (double)a / 2.0 + (double)b / 2.0;
      if (thr == (double)b || isinf(thr)) thr = (double)a;
    }
    s_feat[t] = f;
    s_thr[t] = thr;
    feat_out[h] = f;
    stat_out[h * DCI_STATS] = thr;
  }
  __syncthreads();
  // rows [t chunk, (t + 1) chunk) in order: move, and add to the child's statistics
  double n[NC], sr[NC], srr[NC], sh[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) n[c] = sr[c] = srr[c] = sh[c] = 0.;
#pragma unroll 4
  for (int j = 0; j < chunk; ++j) {
    const int s = t * chunk + j;
    if (s < S) {
      int nd = 0;
      const double rr = w.r[(long)tree * S + s];
      const double p = target_of(labels[s], tree, C) - rr;
      if (L >= 0) {
        nd = w.node[(long)tree * S + s];
        const int at = nd - PBASE;
        if (at >= 0 && at < NP && s_feat[at] >= 0) {
          const float x = table[(rows ? (long)rows[s] : (long)s) * D + s_feat[at]];
          nd = 2 * nd + 1 + ((double)x <= s_thr[at] ? 0 : 1);
          w.node[(long)tree * S + s] = (uint8_t)nd;
        }
      } else {
        w.node[(long)tree * S + s] = 0;
      }
      const int c = nd - CBASE;
      const double h = p * (1. - p);
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (c == k) n[k] += 1., sr[k] += rr, srr[k] += rr * rr, sh[k] += h;
    }
  }
  // every sum over the workgroup: lanes pairwise at distances 32 ... 1, then the waves in order; ONE barrier for all of them
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const double v[4] = {wave_sum(n[c]), wave_sum(sr[c]), wave_sum(srr[c]), wave_sum(sh[c])};
    if ((t & 63) == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s_part[c][i][t >> 6] = v[i];
    }
  }
  __syncthreads();
  if (t < NC) {
    const int c = t, h = CBASE + c;
    double sum[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sum[i] = s_part[c][i][0];
#pragma unroll
      for (int k = 1; k < DCI_WAVES; ++k) sum[i] += s_part[c][i][k];
    }
    const double an = sum[0], asr = sum[1], asrr = sum[2], ash = sum[3];
    const bool open = L + 1 < 3 && an >= 2. && mse_of(an, asr, asrr) > 2.220446049250313e-16;
    double* st = stats + h * DCI_WS_STATS;
    st[0] = an, st[1] = asr, st[2] = asrr, st[3] = ash, st[4] = open ? 1. : 0.;
    stat_out[h * DCI_STATS + 2] = an;
    stat_out[h * DCI_STATS + 3] = asr;
    stat_out[h * DCI_STATS + 4] = asrr;
    if (L == 2) {                                              // depth 3: leaves
      feat_out[h] = -1;
      stat_out[h * DCI_STATS] = 0.;
    }
  }
  if (L < 2) return;
  // the stage ends for this tree: values of all 15 nodes, the raw scores, the importances
  __syncthreads();                                             // this workgroup's stores to stats and tree_feature
  if (t < DCI_NODES) {
    const double* st = stats + t * DCI_WS_STATS;
    const int f = feat_out[t];
    const double nn = st[0];
    double v = 0.;
    if (nn > 0.) {
      v = st[1] / nn;
      if (f < 0) {
        const double num = C == 2 ? v : v * ((double)(C - 1) / (double)C), den = st[3] / nn;
        v = fabs(den) < 1e-150 ? 0. : num / den;
      }
    }
    s_feat[t] = f;
    s_val[t] = v;
#pragma unroll
    for (int i = 0; i < 4; ++i) s_st[t][i] = st[i];
    stat_out[t * DCI_STATS + 1] = v;
  }
  __syncthreads();
  for (int j = 0; j < chunk; ++j) {
    const int s = t * chunk + j;
    if (s >= S) break;
    double* at = raw + (long)s * T + tree;                     // product, then sum: the two roundings k_dci_predict makes
    *at = __dadd_rn(*at, __dmul_rn(learning_rate, s_val[w.node[(long)tree * S + s]]));
  }
  if (t < D) {
    double acc = 0.;
#pragma unroll
    for (int h = 0; h < 7; ++h)
      if (s_feat[h] == t) {
        const int l = 2 * h + 1, r = 2 * h + 2;
        acc += s_st[h][0] * mse_of(s_st[h][0], s_st[h][1], s_st[h][2]) - s_st[l][0] * mse_of(s_st[l][0], s_st[l][1], s_st[l][2]) -
               s_st[r][0] * mse_of(s_st[r][0], s_st[r][1], s_st[r][2]);
      }
    w.imp[((long)stage * T + tree) * D + t] = acc / s_st[0][0];
  }
  if (t == 0) w.split[(long)stage * T + tree] = s_feat[0] >= 0 ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_dci_importance(int D, int S, int T, int n_stages, float* ws, double* __restrict__ importance,
                                                       int32_t* __restrict__ n_split) {
  const int d = threadIdx.x;
  const DciWs w = dci_ws(ws, D, S, T, n_stages);
  const long trees = (long)n_stages * T;
  if (d < D) {
    double acc = 0.;
    for (long i = 0; i < trees; ++i) acc += w.imp[i * D + d];
    importance[d] = acc;
  }
  if (d == 0) {
    int cnt = 0;
    for (long i = 0; i < trees; ++i) cnt += w.split[i];
    n_split[0] = cnt;
  }
}

// ---- predict -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DCI_T) void k_dci_predict(const float* __restrict__ table, const int64_t* __restrict__ rows, int D, long S,
                                                       int T, int n_stages, double learning_rate,
                                                       const int32_t* __restrict__ tree_feature, const double* __restrict__ tree_stats,
                                                       double* __restrict__ raw) {
  const long i = blockIdx.x * (long)DCI_T + threadIdx.x;
  if (i >= S * T) return;
  const long s = i / T;
  const int tree = (int)(i % T);
  const float* x = table + (rows ? (long)rows[s] : s) * D;
  double acc = raw[i];
  for (int stage = 0; stage < n_stages; ++stage) {
    const int32_t* feat = tree_feature + ((long)stage * T + tree) * DCI_NODES;
    const double* st = tree_stats + ((long)stage * T + tree) * DCI_NODES * DCI_STATS;
    int h = 0;
#pragma unroll
    for (int depth = 0; depth < 3; ++depth) {
      const int f = feat[h];
      if (f >= 0) h = 2 * h + 1 + ((double)x[f] <= st[h * DCI_STATS] ? 0 : 1);
    }
    acc = __dadd_rn(acc, __dmul_rn(learning_rate, st[h * DCI_STATS + 1]));
  }
  raw[i] = acc;
}

bool sizes_ok(long N, int D, long S, int C, int n_stages) {
  return N > 0 && N <= 2147483647L && D > 0 && D <= DVAE_DCI_MAX_D && S > 0 && S <= DVAE_DCI_MAX_ROWS && C > 0 &&
         C <= DVAE_DCI_MAX_CLASSES && n_stages > 0 && n_stages <= DVAE_DCI_MAX_STAGES;
}

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_dci_version(void) { return DVAE_DCI_VERSION; }
const char* dvae_dci_last_error(void) { return last_error(); }
int dvae_dci_trees(int C) { return C > 0 && C <= DVAE_DCI_MAX_CLASSES ? trees_of(C) : 0; }

size_t dvae_dci_fit_ws_floats(long N, int D, long S, int C, int n_stages) {
  if (S <= 0) S = N;
  if (!sizes_ok(N, D, S, C, n_stages)) return 0;
  return dci_ws_floats(D, (int)S, trees_of(C), n_stages);
}

int dvae_dci_fit(const float* table, const int64_t* rows, const int32_t* order, const int32_t* labels, long N, int D, long S, int C,
                 int n_stages, double learning_rate, int init, double* raw, double* prior, float* ws, double* importance,
                 int32_t* n_split, int32_t* tree_feature, double* tree_stats, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && order && labels && raw && prior && ws && importance && n_split && tree_feature && tree_stats);
  DVAE_CHECK_ARG(D <= DVAE_DCI_MAX_D);
  DVAE_CHECK_ARG(S <= DVAE_DCI_MAX_ROWS);
  DVAE_CHECK_ARG(C <= DVAE_DCI_MAX_CLASSES);
  DVAE_CHECK_ARG(sizes_ok(N, D, S, C, n_stages));
  DVAE_CHECK_ARG(learning_rate > 0. && learning_rate <= 1.);
  DVAE_CHECK_ARG(init == 0 || init == 1);
  DVAE_CHECK_ARG(((uintptr_t)ws & 7u) == 0);
  hipStream_t st = (hipStream_t)stream;
  const int Si = (int)S, T = trees_of(C);
  const int chunk = (Si + DCI_T - 1) / DCI_T;
  const size_t lds = (size_t)DVAE_DCI_ROW_LDS_BYTES * chunk * DCI_T;
  // above 64 KB of dynamic LDS a kernel must be allowed it: asked for once, for the largest size, so that no size takes another path
  static const hipError_t allowed =
      hipFuncSetAttribute((const void*)k_dci_search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DCI_LDS_MAX);
  if (allowed != hipSuccess) {
    set_error("%s:%d: %d bytes of dynamic LDS refused for k_dci_search: %s", __FILE__, __LINE__, (int)DCI_LDS_MAX,
              hipGetErrorString(allowed));
    return -2;
  }
  const DciWs w = dci_ws(ws, D, Si, T, n_stages);
  const dim3 block(DCI_T), per_tree(T), per_pair(D, T), per_row((Si + DCI_T - 1) / DCI_T);
  hipLaunchKernelGGL(k_dci_prior, dim3(1), block, 0, st, labels, Si, C, prior);
  DVAE_CHECK_LAUNCH();
  if (init) {
    hipLaunchKernelGGL(k_dci_fill_raw, dim3((unsigned)(((long)Si * T + DCI_T - 1) / DCI_T)), block, 0, st, prior, Si, T, raw);
    DVAE_CHECK_LAUNCH();
  }
  for (int stage = 0; stage < n_stages; ++stage) {
    hipLaunchKernelGGL(k_dci_residual, per_row, block, 0, st, labels, raw, Si, C, T, w.r);
    DVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_dci_split<-1>, per_tree, block, 0, st, table, rows, labels, D, Si, chunk, C, T, n_stages, stage, learning_rate,
                       ws, raw, tree_feature, tree_stats);
    DVAE_CHECK_LAUNCH();
    for (int level = 0; level < 3; ++level) {
      hipLaunchKernelGGL(k_dci_search, per_pair, block, lds, st, table, rows, order, D, Si, chunk, level, T, n_stages, ws);
      DVAE_CHECK_LAUNCH();
      if (level == 0)
        hipLaunchKernelGGL(k_dci_split<0>, per_tree, block, 0, st, table, rows, labels, D, Si, chunk, C, T, n_stages, stage,
                           learning_rate, ws, raw, tree_feature, tree_stats);
      else if (level == 1)
        hipLaunchKernelGGL(k_dci_split<1>, per_tree, block, 0, st, table, rows, labels, D, Si, chunk, C, T, n_stages, stage,
                           learning_rate, ws, raw, tree_feature, tree_stats);
      else
        hipLaunchKernelGGL(k_dci_split<2>, per_tree, block, 0, st, table, rows, labels, D, Si, chunk, C, T, n_stages, stage,
                           learning_rate, ws, raw, tree_feature, tree_stats);
      DVAE_CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(k_dci_importance, dim3(1), dim3(64), 0, st, D, Si, T, n_stages, ws, importance, n_split);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_dci_predict(const float* table, const int64_t* rows, long N, int D, long S, int C, int n_stages, double learning_rate,
                     const int32_t* tree_feature, const double* tree_stats, double* raw, void* stream) {
  if (!rows) S = N;
  DVAE_CHECK_ARG(table && tree_feature && tree_stats && raw);
  DVAE_CHECK_ARG(D <= DVAE_DCI_MAX_D);
  DVAE_CHECK_ARG(C <= DVAE_DCI_MAX_CLASSES);
  DVAE_CHECK_ARG(N > 0 && N <= 2147483647L && D > 0 && S > 0 && S <= 2147483647L && C > 0 && n_stages > 0 &&
                 n_stages <= DVAE_DCI_MAX_STAGES);
  DVAE_CHECK_ARG(learning_rate > 0. && learning_rate <= 1.);
  const int T = trees_of(C);
  const long work = S * T;
  hipLaunchKernelGGL(k_dci_predict, dim3((unsigned)((work + DCI_T - 1) / DCI_T)), dim3(DCI_T), 0, (hipStream_t)stream, table, rows, D,
                     S, T, n_stages, learning_rate, tree_feature, tree_stats, raw);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
