// Target elements of the reconstruction likelihood as unit floats: shared by the convT3 forward kernels (conv_thin.hip,
// conv_up_thin_mm.hip), the input staging of conv_thin.hip and the per-image scores (loglik.hip).  The per-element step and
// the workgroup tail of the three convT3 kernels stay in the kernels: routed through shared helpers, the compiler emitted
// different code for k_up_thin / k_up_thin_pk (a commuted address add and renamed registers for the tail alone; other
// schedules for the element step), and sharing them is only worth a change that is measured on its own.
#pragma once
#include "common.h"

namespace dvae {

// Image elements: fp32, or uint8 pixels as the datasets store them (dSprites imgs * 255, CelebA imread:
// utils/datasets.py:204-213,282-291) converted on the fly with ToTensor's arithmetic, float(v) / 255 (IEEE
// division: bit-identical to torchvision's .div(255)).  The batch then stays uint8 in HBM: the kernels that read the
// input image (conv1 forward, conv1 weight gradient, reconstruction likelihood) fetch 1 byte per pixel.
__device__ __forceinline__ float to_unit(float v) { return v; }
__device__ __forceinline__ float to_unit(uint8_t v) { return (float)v / 255.0f; }
// the same for an element of type TT that already travels as a float (k_up_thin_pk converts where it loads, divides where
// it consumes)
template <typename TT>
__device__ __forceinline__ float raw_to_unit(float v) {
  if constexpr (sizeof(TT) == 4) return v;
  else return v / 255.0f;
}

// quad q of a target -> fp32
__device__ __forceinline__ f32x4 target_quad(const void* __restrict__ target, int u8, long q) {
  f32x4 t;
  if (u8) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(target)[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = (float)((w >> (8 * j)) & 0xff) / 255.0f;      // = to_unit of byte j
  } else {
    t = reinterpret_cast<const f32x4*>(target)[q];
  }
  return t;
}

}  // namespace dvae
