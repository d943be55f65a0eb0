// Image grid of a decoded batch as uint8 RGB (the visualizer's pictures: utils/visualize.py:124-135 -- F.interpolate(nearest) +
// torchvision make_grid + make_grid_img / save_image -- in ONE launch on the device, so that only the uint8 grid crosses to the
// host).  Semantics restated in include/dvae_hip.h (dvae_image_grid_u8).
#include "common.h"

namespace dvae {

namespace {

struct GridGeom {
  long n;          // images
  int C, H, W;     // input geometry (C = 1 is replicated to RGB)
  int f;           // nearest-neighbour upsampling factor
  int pad;         // padding (0 when n == 1: make_grid returns the single image)
  int xmaps;       // images per grid row
  long gh, gw;     // grid height / width
};

__device__ __forceinline__ uint32_t to_u8(float v) {
  // grid.mul(255).add_(0.5).clamp_(0, 255) -> uint8: two fp32 roundings (no FMA), clamp, truncation toward zero.  The product and
  // the sum are written out under contract(off): __fmul_rn / __fadd_rn are plain operators in this toolchain's headers, and
  // -ffp-contract=fast fuses them into one v_fma_f32 (a different rounding of k + 0.5 +- 1 ulp).
#pragma clang fp contract(off)
  const float m = v * 255.0f;
  v = m + 0.5f;
  v = fminf(fmaxf(v, 0.0f), 255.0f);
  return (uint32_t)v;
}

// byte `b` of the HWC RGB grid, given its pixel coordinates (gy, gx) and channel c
__device__ __forceinline__ uint32_t grid_byte(const float* __restrict__ imgs, const GridGeom& g, long gy, long gx, int c,
                                              uint32_t pad_u8) {
  const long hs = (long)g.H * g.f, ws = (long)g.W * g.f;
  const long ty = gy - g.pad, tx = gx - g.pad;
  if (ty < 0 || tx < 0) return pad_u8;
  const long cy = ty / (hs + g.pad), cx = tx / (ws + g.pad);
  const long iy = ty - cy * (hs + g.pad), ix = tx - cx * (ws + g.pad);
  if (iy >= hs || ix >= ws || cx >= g.xmaps) return pad_u8;
  const long k = cy * g.xmaps + cx;
  if (k >= g.n) return pad_u8;
  const int ch = g.C == 1 ? 0 : c;
  return to_u8(imgs[((k * g.C + ch) * g.H + iy / g.f) * (long)g.W + ix / g.f]);
}

// One thread per 16 output bytes (grid-stride): a 16-byte store where the run is whole and aligned, byte stores otherwise.
__global__ __launch_bounds__(256) void k_image_grid_u8(const float* __restrict__ imgs, GridGeom g, float pad_value,
                                                       uint8_t* __restrict__ out) {
  const long total = g.gh * g.gw * 3;
  const uint32_t pad_u8 = to_u8(pad_value);
  const bool aligned = ((uintptr_t)out & 15) == 0;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q * 16 < total; q += (long)gridDim.x * blockDim.x) {
    const long b0 = q * 16;
    const long p0 = b0 / 3;
    int c = (int)(b0 - p0 * 3);
    long gy = p0 / g.gw, gx = p0 - gy * g.gw;
    if (aligned && b0 + 16 <= total) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        w[j >> 2] |= grid_byte(imgs, g, gy, gx, c, pad_u8) << (8 * (j & 3));
        if (++c == 3) {
          c = 0;
          if (++gx == g.gw) {
            gx = 0;
            ++gy;
          }
        }
      }
      *reinterpret_cast<uint4*>(out + b0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (long b = b0; b < total && b < b0 + 16; ++b) {
        out[b] = (uint8_t)grid_byte(imgs, g, gy, gx, c, pad_u8);
        if (++c == 3) {
          c = 0;
          if (++gx == g.gw) {
            gx = 0;
            ++gy;
          }
        }
      }
    }
  }
}

}  // namespace

int image_grid_geom(long n, int H, int W, int nrow, int padding, int upsample, long* gh, long* gw, int* xmaps, int* pad) {
  const int p = n == 1 ? 0 : padding;
  const long xm = n < nrow ? n : nrow;
  const long ym = (n + xm - 1) / xm;
  const long h = ym * ((long)H * upsample + p) + p, w = xm * ((long)W * upsample + p) + p;
  if (h <= 0 || w <= 0 || h > (1L << 24) || w > (1L << 24) || h * w > (1L << 40) / 3) return -1;
  *gh = h;
  *gw = w;
  *xmaps = (int)xm;
  *pad = p;
  return 0;
}

int launch_image_grid_u8(const float* imgs, long n, int C, int H, int W, int nrow, int padding, float pad_value, int upsample,
                         uint8_t* out, hipStream_t s) {
  GridGeom g{n, C, H, W, upsample, 0, 0, 0, 0};
  if (image_grid_geom(n, H, W, nrow, padding, upsample, &g.gh, &g.gw, &g.xmaps, &g.pad) != 0) {
    set_error("dvae_image_grid_u8: grid of %ld images of %dx%d (nrow %d, padding %d, upsample %d) is too large", n, H, W, nrow,
              padding, upsample);
    return -1;
  }
  const long runs = (g.gh * g.gw * 3 + 15) / 16;
  long blocks = (runs + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_image_grid_u8, dim3((unsigned)blocks), dim3(256), 0, s, imgs, g, pad_value, out);
  DVAE_CHECK_LAUNCH();
  return 0;
}

}  // namespace dvae
