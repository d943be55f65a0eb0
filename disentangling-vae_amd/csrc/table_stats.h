// Helpers shared by the score libraries that scan the [N, D] table of posterior means (factor_scores.hip, factor_info.hip,
// factor_irs.hip, latent_pairs.hip): the ONE definition in csrc/ of each.  Every library keeps its own named kernels; what is
// here is inlined into them.  As in latent_math.h the operation order of every helper is part of its contract, and a change
// here is gated on the machine code of its callers (tools/isa_identity.py).  Two pieces that the kernels repeat are NOT here,
// because every shared form of them changed the machine code of a caller: the count of histogram edges <= x (k_info_joint_hist,
// k_unsup_pair_hist) and the sizes / saturating strides of the factors (load_factors of factor_info.hip, load_factor of
// factor_irs.hip); each site says so.  Not included by common.h: the training library uses none of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dvae {

template <class T>
__host__ __device__ __forceinline__ T lesser(T a, T b) { return a < b ? a : b; }

// doubles cross the fp32 workspace as two words: ws is aligned to 4 bytes and no more
__device__ __forceinline__ void put_f64(float* p, double v) {
  p[0] = __int_as_float(__double2loint(v));
  p[1] = __int_as_float(__double2hiint(v));
}
__device__ __forceinline__ double get_f64(const float* p) { return __hiloint2double(__float_as_int(p[1]), __float_as_int(p[0])); }

// chunks of the S rows: ceil(S / block_rows) workgroups, at most max_blocks, none of them empty
static inline int chunks_of(long S, long block_rows, long max_blocks, long* chunk) {
  long nb = (S + block_rows - 1) / block_rows;
  if (nb > max_blocks) nb = max_blocks;
  *chunk = (S + nb - 1) / nb;
  return (int)((S + *chunk - 1) / *chunk);
}

// lanes that read one row of D floats: D padded to 4 / 16 / 64 (D > 64 walks the row in pieces of 64)
static inline int padded_width(int D) { return D <= 4 ? 4 : D <= 16 ? 16 : 64; }

// body of a library's own k_*_zero kernel: a grid-stride clear by workgroups of T threads
template <int T>
__device__ __forceinline__ void zero_i32(int32_t* __restrict__ p, long n) {
  for (long i = blockIdx.x * (long)T + threadIdx.x; i < n; i += (long)gridDim.x * T) p[i] = 0;
}

}  // namespace dvae
