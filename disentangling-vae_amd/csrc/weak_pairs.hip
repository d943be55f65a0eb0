// libdvae_weak_hip.so (include/dvae_weak_hip.h): the adaptive group posterior of Ada-GVAE / Ada-ML-VAE (Locatello et al. 2020) on
// a batch of image pairs -- rows i and P + i of the interleaved [2 P, 2 D] output of mu_logvar_gen -- and its backward pass.  A
// TRAINING plugin: the two launches sit around dvae_reparam_kl_fwd / dvae_reparam_kl_bwd in WeakVaeLoss's step.  Both are a few
// flops per element on 16 P D bytes: launch-bound at every batch size of the project.
//
// k_weak_fwd<KIND>.  A pair owns G = D rounded up to a power of two consecutive lanes of ONE wave (G <= 64: 64 / G pairs per wave,
// 256 / G per workgroup); lane d of the group loads the couples (mu_a, lv_a), (mu_b, lv_b) of dimension d -- consecutive 8-byte
// words along the row -- and computes delta.  max_d and min_d are a butterfly of log2 G cross-lane exchanges (__shfl_xor with
// offsets G / 2 .. 1: the lanes of a group differ in their low log2 G bits only, so an exchange never leaves the group); padding
// lanes enter with -inf / +inf.  Every lane of a group ends with the same two values, whatever D is: the tree is fixed.  The
// mask word is the group's slice of the wave's ballot, stored by lane 0 of the group.  A shared element is computed once by its
// lane and stored to both rows.
//
// k_weak_bwd<KIND>.  Thread (pair, d) reads the mask word of its pair and, where bit d is set, replaces the two gradient couples in
// place.  No reduction.
//
// No atomics, no LDS, no cooperative launch, no loop whose bound is not a function of the arguments.
#include "../../include/dvae_weak_hip.h"
#include "common.h"
#include "last_error.h"

namespace dvae {

namespace {

#define WEAK_T DVAE_WEAK_THREADS
#define WEAK_LOG2 0.69314718055994531f

static_assert(WEAK_T % 64 == 0 && DVAE_WEAK_MAX_D == 64, "a pair's lanes lie in one wave and its mask is one word");

// log(1 + exp(-|t|)): in (0, log 2]
__device__ __forceinline__ float softplus_neg_abs(float t) { return log1pf(expf(-fabsf(t))); }

// the aggregated (m, lv~) of one shared element; t = lv_b - lv_a
template <int KIND>
__device__ __forceinline__ float2 aggregate(float2 a, float2 b) {
  const float t = b.y - a.y;
  const float sp = softplus_neg_abs(t);
  float2 r;
  if (KIND == DVAE_WEAK_GVAE) {
    r.x = 0.5f * (a.x + b.x);
    r.y = (fmaxf(a.y, b.y) + sp) - WEAK_LOG2;
  } else {
    const float wa = 1.f / (1.f + expf(-t)), wb = 1.f / (1.f + expf(t));
    r.x = wa * a.x + wb * b.x;
    r.y = (WEAK_LOG2 + fminf(a.y, b.y)) - sp;
  }
  return r;
}

template <int KIND>
__global__ __launch_bounds__(WEAK_T) void k_weak_fwd(const float2* __restrict__ ml, long pairs, int D, int G,
                                                     float2* __restrict__ ml_agg, unsigned long long* __restrict__ shared,
                                                     float* __restrict__ delta) {
  const int t = threadIdx.x;
  const long gl = (long)blockIdx.x * WEAK_T + t;
  const int d = (int)(gl & (G - 1));
  const long pair = gl / G;
  const bool valid = pair < pairs && d < D;
  float2 a = {0.f, 0.f}, b = {0.f, 0.f};
  float dl = 0.f;
  if (valid) {
    a = ml[pair * D + d];
    b = ml[(pair + pairs) * D + d];
    const float dm = b.x - a.x;
    dl = ((expf(a.y - b.y) + dm * dm * expf(-b.y)) - 1.f) + (b.y - a.y);
  }
  float hi = valid ? dl : -INFINITY, lo = valid ? dl : INFINITY;
  for (int o = G >> 1; o > 0; o >>= 1) {                                 // (uniform: every lane of the wave takes part)
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    lo = fminf(lo, __shfl_xor(lo, o, 64));
  }
  const float tau = 0.5f * hi + 0.5f * lo;
  const bool sh = valid && dl < tau;
  const unsigned long long vote = __ballot(sh);
  if (!valid) return;
  if (d == 0) {
    const int shift = (t & 63) & ~(G - 1);
    shared[pair] = (vote >> shift) & (G == 64 ? ~0ull : ((1ull << G) - 1ull));
  }
  if (delta) delta[pair * D + d] = dl;
  if (sh) a = b = aggregate<KIND>(a, b);
  ml_agg[pair * D + d] = a;
  ml_agg[(pair + pairs) * D + d] = b;
}

template <int KIND>
__global__ __launch_bounds__(WEAK_T) void k_weak_bwd(const float2* __restrict__ ml, const unsigned long long* __restrict__ shared,
                                                     long pairs, int D, float2* __restrict__ dml) {
  const long i = (long)blockIdx.x * WEAK_T + threadIdx.x;               // element (pair, d)
  if (i >= pairs * D) return;
  const long pair = i / D;
  const int d = (int)(i - pair * D);
  if (!((shared[pair] >> d) & 1ull)) return;
  const long ia = i, ib = i + pairs * D;
  const float2 a = ml[ia], b = ml[ib];
  const float2 ga = dml[ia], gb = dml[ib];
  const float gm = ga.x + gb.x, gl = ga.y + gb.y;
  const float t = b.y - a.y;
  const float wa = 1.f / (1.f + expf(-t)), wb = 1.f / (1.f + expf(t));   // sigmoid(lv_b - lv_a), sigmoid(lv_a - lv_b)
  float2 ra, rb;
  if (KIND == DVAE_WEAK_GVAE) {
    ra.x = rb.x = 0.5f * gm;
    ra.y = gl * wb;
    rb.y = gl * wa;
  } else {
    const float c = gm * (wa * wb) * (a.x - b.x);
    ra.x = gm * wa;
    rb.x = gm * wb;
    ra.y = gl * wa - c;
    rb.y = gl * wb + c;
  }
  dml[ia] = ra;
  dml[ib] = rb;
}

// D rounded up to a power of two: the lanes of a pair
int group_of(int D) {
  int g = 1;
  for (int k = 0; k < 6 && g < D; ++k) g <<= 1;
  return g;
}

bool sizes_ok(long pairs, int D) { return pairs >= 1 && pairs <= DVAE_WEAK_MAX_PAIRS && D >= 1 && D <= DVAE_WEAK_MAX_D; }

}  // namespace
}  // namespace dvae

using namespace dvae;

extern "C" {

int dvae_weak_version(void) { return DVAE_WEAK_VERSION; }
const char* dvae_weak_last_error(void) { return last_error(); }

int dvae_weak_aggregate_fwd(const float* ml, long pairs, int D, int kind, float* ml_agg, uint64_t* shared, float* delta,
                            void* stream) {
  DVAE_CHECK_ARG(ml && ml_agg && shared);
  DVAE_CHECK_ARG(D <= DVAE_WEAK_MAX_D);
  DVAE_CHECK_ARG(pairs <= DVAE_WEAK_MAX_PAIRS);
  DVAE_CHECK_ARG(sizes_ok(pairs, D));
  DVAE_CHECK_ARG(kind == DVAE_WEAK_GVAE || kind == DVAE_WEAK_MLVAE);
  const int G = group_of(D);
  const int blocks = (int)((pairs * G + WEAK_T - 1) / WEAK_T);
  const auto kern = kind == DVAE_WEAK_GVAE ? k_weak_fwd<DVAE_WEAK_GVAE> : k_weak_fwd<DVAE_WEAK_MLVAE>;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(WEAK_T), 0, (hipStream_t)stream, (const float2*)ml, pairs, D, G, (float2*)ml_agg,
                     (unsigned long long*)shared, delta);
  DVAE_CHECK_LAUNCH();
  return 0;
}

int dvae_weak_aggregate_bwd(const float* ml, const uint64_t* shared, long pairs, int D, int kind, float* dml, void* stream) {
  DVAE_CHECK_ARG(ml && shared && dml);
  DVAE_CHECK_ARG(D <= DVAE_WEAK_MAX_D);
  DVAE_CHECK_ARG(pairs <= DVAE_WEAK_MAX_PAIRS);
  DVAE_CHECK_ARG(sizes_ok(pairs, D));
  DVAE_CHECK_ARG(kind == DVAE_WEAK_GVAE || kind == DVAE_WEAK_MLVAE);
  const int blocks = (int)((pairs * D + WEAK_T - 1) / WEAK_T);
  const auto kern = kind == DVAE_WEAK_GVAE ? k_weak_bwd<DVAE_WEAK_GVAE> : k_weak_bwd<DVAE_WEAK_MLVAE>;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(WEAK_T), 0, (hipStream_t)stream, (const float2*)ml, (const unsigned long long*)shared,
                     pairs, D, (float2*)dml);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
