// What dy_process_mask (mask_ops.hip) and dy_val_mask_match (val_mask.hip) share, so that a prediction's mask is the same set of proto
// pixels in both: the crop window of ops.crop_mask at proto resolution and the 32-term fp32 dot product of one 128-byte proto pixel.
#pragma once
#include "common_hip.h"

namespace dy {

struct CropWin {  // inclusive bounds in grid pixels; empty when lo > hi
  int x_lo, x_hi, y_lo, y_hi;
};

// crop_mask on a (sh, sw) grid: pixel (yy, xx) is kept iff x1 <= xx < x2 and y1 <= yy < y2 (the corners already in grid pixels; clamped
// through float so that huge boxes cannot overflow the int conversion).  crop_mask compares: a NaN corner is inside no inequality, the
// window is empty (fmaxf would turn a NaN x1 / y1 into column / row 0).
__device__ __forceinline__ CropWin crop_window(float x1, float y1, float x2, float y2, int sw, int sh) {
  CropWin c;
  c.x_lo = (int)ceilf(fminf(fmaxf(x1, 0.f), (float)sw));
  c.x_hi = (int)ceilf(fminf(fmaxf(x2, 0.f), (float)sw)) - 1;
  c.y_lo = (int)ceilf(fminf(fmaxf(y1, 0.f), (float)sh));
  c.y_hi = (int)ceilf(fminf(fmaxf(y2, 0.f), (float)sh)) - 1;
  if (!(x1 == x1 && x2 == x2 && y1 == y1 && y2 == y2)) c.x_hi = c.x_lo - 1;
  return c;
}

// sum_k cf[k] * px[k] over one proto pixel (32 fp32 = 8 x 16-byte loads of one lane), one fma chain in channel order
__device__ __forceinline__ float proto_dot32(const float (&cf)[32], const float* px) {
  const f32x4* p = reinterpret_cast<const f32x4*>(px);
  float v = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 t = p[q];
    v = __builtin_fmaf(cf[4 * q + 0], t[0], v);
    v = __builtin_fmaf(cf[4 * q + 1], t[1], v);
    v = __builtin_fmaf(cf[4 * q + 2], t[2], v);
    v = __builtin_fmaf(cf[4 * q + 3], t[3], v);
  }
  return v;
}

// What dy_process_mask and dy_tile_process_mask (mask_ops.hip) share, so that a frame mask at stride 1 is the tile's mask bit for bit.
// Source coordinate of PyTorch's bilinear resize (align_corners = False) for the output pixel whose CENTRE is at `centre` (dst + 0.5
// in output pixels): scale * centre - 0.5, clamped at 0.
__device__ __forceinline__ float pm_src_at(float scale, float centre) {
  const float s = scale * centre - 0.5f;
  return s < 0.f ? 0.f : s;
}

// The blend of the four corner values (top / bottom row, left / right column) with the weights of the two rows and the two columns.
__device__ __forceinline__ float pm_blend(float ly0, float ly1, float lx0, float lx1, float tl, float tr, float bl, float br) {
  return ly0 * (lx0 * tl + lx1 * tr) + ly1 * (lx0 * bl + lx1 * br);
}

}  // namespace dy
