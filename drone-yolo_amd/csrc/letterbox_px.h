// The one copy of the 8-bit bilinear arithmetic of LetterBox's resize (OpenCV INTER_LINEAR, 11-bit fixed-point coefficients, restated in
// oracle/letterbox_oracle.py), shared by dy_letterbox_u8_to_nchw_f32 (preproc.hip: whole frames) and dy_crops_letterbox_u8_to_nchw_f32
// (pose.hip: windows of frames).  A source is a window of h0 x w0 pixels whose rows lie `pitch` bytes apart: a whole frame has
// pitch = w0 * 3, a crop the pitch of the frame it is cut from.
#pragma once
#include "common_hip.h"

namespace dy {

__device__ __forceinline__ void axis_coeff(int d, double scale, int src, int* s0, int* s1, int* a0, int* a1) {
  // unfused double arithmetic so that the result equals numpy's (oracle): (d + 0.5) * scale - 0.5
  double f = __dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
  int s = (int)floor(f);
  f = f - (double)s;
  if (s < 0) f = 0.0, s = 0;
  if (s >= src - 1) f = 0.0, s = src - 1;
  const float ff = (float)f;
  *a0 = (int)rintf(__fmul_rn(__fsub_rn(1.0f, ff), 2048.0f));
  *a1 = (int)rintf(__fmul_rn(ff, 2048.0f));
  *s0 = s;
  *s1 = s + 1 < src ? s + 1 : src - 1;
}

// The vertical half of a resized pixel: rows and weights of output row ry.
struct LbRow {
  int y0, y1, by0, by1;
};

__device__ __forceinline__ LbRow letterbox_row(int ry, double sy, int h0) {
  LbRow r;
  axis_coeff(ry, sy, h0, &r.y0, &r.y1, &r.by0, &r.by1);
  return r;
}

// Pixel (ry, rx) of the window `s` resized to (new_h, new_w); v: the three channels as floats in [0, 255].  new size == window size copies.
__device__ __forceinline__ void letterbox_px(const uint8_t* s, size_t pitch, int h0, int w0, int new_h, int new_w, double sx, const LbRow& row, int ry,
                                             int rx, float v[3]) {
  if (new_h == h0 && new_w == w0) {
    const uint8_t* q = s + (size_t)ry * pitch + (size_t)rx * 3;
    v[0] = (float)q[0], v[1] = (float)q[1], v[2] = (float)q[2];
    return;
  }
  int x0, x1, ax0, ax1;
  axis_coeff(rx, sx, w0, &x0, &x1, &ax0, &ax1);
  const uint8_t* r0 = s + (size_t)row.y0 * pitch;
  const uint8_t* r1 = s + (size_t)row.y1 * pitch;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0v = (int)r0[x0 * 3 + c] * ax0 + (int)r0[x1 * 3 + c] * ax1;
    const int h1v = (int)r1[x0 * 3 + c] * ax0 + (int)r1[x1 * 3 + c] * ax1;
    int o = (((row.by0 * (h0v >> 4)) >> 16) + ((row.by1 * (h1v >> 4)) >> 16) + 2) >> 2;
    o = o < 0 ? 0 : (o > 255 ? 255 : o);
    v[c] = (float)o;
  }
}

}  // namespace dy
