/*
 * libdvae_weak_hip.so -- C-ABI of the MI355X (gfx950) kernels behind the weakly-supervised pair losses Ada-GVAE / Ada-ML-VAE
 * (Locatello et al. 2020, "Weakly-Supervised Disentanglement Without Compromises"; disentanglement_lib's weak_vae.py): the
 * adaptive group posterior of a batch of image PAIRS and its backward pass.  A library of its own next to libdvae_hip.so
 * (include/dvae_hip.h), the score libraries and the two other loss plugins (libdvae_dip_hip.so, libdvae_mmd_hip.so); nothing of it
 * is linked into another.  Like those two it IS part of the training step: WeakVaeLoss (disvae_amd/models/losses.py) issues
 * dvae_weak_aggregate_fwd between mu_logvar_gen and dvae_reparam_kl_fwd, and dvae_weak_aggregate_bwd behind dvae_reparam_kl_bwd.
 * The reference (YannDubs/disentangling-vae) has no counterpart.
 *
 * A batch has 2 P rows; rows i and P + i are pair i (a = row i, b = row P + i).  ml [2 P, 2 D] is the interleaved output of
 * mu_logvar_gen (mu = ml[:, 0::2], lv = ml[:, 1::2]: what dvae_reparam_kl_fwd consumes and dvae_reparam_kl_bwd produces).
 *   delta[i,d] = exp(lv_a - lv_b) + (mu_b - mu_a)^2 exp(-lv_b) - 1 + (lv_b - lv_a)          (2 KL(q_a || q_b) per dimension)
 *   tau[i]     = 0.5 max_d delta[i,d] + 0.5 min_d delta[i,d]                                 (min / max skip a NaN: fminf / fmaxf)
 *   shared     : delta[i,d] < tau[i], strictly (D = 1 or all delta equal: nothing; a NaN compares false)
 * On a shared dimension both rows receive the same (m, lv~); elsewhere each row keeps its own values.  With t = lv_b - lv_a:
 *   DVAE_WEAK_GVAE   m = (mu_a + mu_b) / 2                    lv~ = max(lv_a, lv_b) + log1p(exp(-|t|)) - log 2
 *   DVAE_WEAK_MLVAE  m = w mu_a + (1 - w) mu_b, w = 1 / (1 + exp(-t)), 1 - w = 1 / (1 + exp(t))
 *                                                             lv~ = log 2 + min(lv_a, lv_b) - log1p(exp(-|t|))
 * The mask is a constant for the gradient.  Backward, with G_m / G_l the sums of the pair's two gradients with respect to m / lv~:
 *   GVAE    dmu_a = dmu_b = G_m / 2;  dlv_a = G_l / (1 + exp(t));  dlv_b = G_l / (1 + exp(-t))
 *   MLVAE   dmu_a = G_m w;  dmu_b = G_m (1 - w);  c = G_m w (1 - w) (mu_a - mu_b);  dlv_a = G_l w - c;  dlv_b = G_l (1 - w) + c
 *
 * Conventions:
 *   - ml, ml_agg, dml are DEVICE pointers to fp32 aligned to 8 bytes (a (mu, lv) couple is one access); delta to fp32 aligned to 4
 *     bytes; shared to 64-bit words aligned to 8 bytes; sizes are element counts;
 *   - 1 <= D <= DVAE_WEAK_MAX_D (the mask of a pair is ONE word), 1 <= pairs <= DVAE_WEAK_MAX_PAIRS, kind one of DVAE_WEAK_GVAE /
 *     DVAE_WEAK_MLVAE; anything else returns <0 (text via dvae_weak_last_error(), per thread) before any launch;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work: no allocation, no synchronisation, no copy;
 *   - all arithmetic is fp32 in a fixed order; min and max over d are a butterfly of cross-lane exchanges over the lanes of a
 *     pair (D rounded up to a power of two); there are no atomics: the same inputs give the same bits on every run.
 */
#ifndef DVAE_WEAK_HIP_H
#define DVAE_WEAK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVAE_WEAK_VERSION 1

/* D above DVAE_WEAK_MAX_D and pairs above DVAE_WEAK_MAX_PAIRS are refused                                                     */
#define DVAE_WEAK_MAX_D 64
#define DVAE_WEAK_MAX_PAIRS 16777216
/* the `kind` argument                                                                                                         */
#define DVAE_WEAK_GVAE 0
#define DVAE_WEAK_MLVAE 1
/* a workgroup: four waves.  The forward launch gives a pair G consecutive lanes of one wave, G = D rounded up to a power of
 * two, so a workgroup owns DVAE_WEAK_THREADS / G pairs                                                                         */
#define DVAE_WEAK_THREADS 256

int dvae_weak_version(void);
const char* dvae_weak_last_error(void);

/* ---- forward ------------------------------------------------------------------------------------------------------------------
 *   ml       fp32 [2 pairs, 2 D]  IN
 *   ml_agg   fp32 [2 pairs, 2 D]  OUT: the aggregated posterior, same layout; every element is written.  The value of a shared
 *            dimension is computed ONCE and stored to both rows: they hold the same bits
 *   shared   64-bit words [pairs] OUT: bit d set when dimension d of the pair is shared; bits >= D are 0
 *   delta    fp32 [pairs, D]      OUT or NULL (tests, logging)                                                                 */
int dvae_weak_aggregate_fwd(const float* ml, long pairs, int D, int kind, float* ml_agg, uint64_t* shared, float* delta,
                            void* stream);

/* ---- backward -----------------------------------------------------------------------------------------------------------------
 *   ml, shared  what the forward launch read and wrote for the SAME pairs, D, kind
 *   dml         fp32 [2 pairs, 2 D] IN-OUT: on entry the gradient with respect to ml_agg (dvae_reparam_kl_bwd's output), on exit
 *               the gradient with respect to ml.  One thread owns element (pair, d) of BOTH rows: the update is in place.  An
 *               element of a dimension that is not shared is left as it is                                                     */
int dvae_weak_aggregate_bwd(const float* ml, const uint64_t* shared, long pairs, int D, int kind, float* dml, void* stream);

#ifdef __cplusplus
}
#endif
#endif
