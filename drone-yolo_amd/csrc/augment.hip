// Training augmentation, one kernel (dy_augment_u8_nchw; include/dyolo.h has the contract):
//   Mosaic._mosaic4 paste (ultralytics/data/augment.py:684-708) -> RandomPerspective warp (augment.py:1041-1078, borderValue 114)
//   -> RandomHSV look-ups (augment.py:1379-1388) -> RandomFlip (augment.py:1464-1481), as ONE gather per output pixel.
// The reference pastes four images onto a 2S x 2S canvas and warps the canvas; here an output pixel is mapped back through the inverse
// matrix to a canvas coordinate and each of its four bilinear neighbours is read straight from the source rectangle that covers it, so
// the canvas never exists.  cv2's fixed-point warpAffine / cvtColor are not restated (cv2 is not available to pin them): interpolation is
// fp32 bilinear and the colour conversion fp32 with integer H, S, V in cv2's 8-bit ranges.
// Shape: a pure gather, bound by the memory system.  One thread makes four horizontally adjacent pixels and stores one packed 32-bit word
// per colour plane (lane-contiguous: a wave writes 256 consecutive bytes of a row); blockIdx.y is the output image, so the table row is
// wave-uniform and lives in scalar registers.  No LDS, no atomics.
#include "common_hip.h"

namespace dy {

struct AugArgs {
  const uint8_t* src;
  const dy_aug_row* table;
  uint8_t* dst;
  int n, hs, ws, batch, s;
};

// the canvas pixel (cx, cy): the source rectangle that covers it (the last one pasted wins, as the paste order has it), else 114
__device__ __forceinline__ void canvas_px(const AugArgs& p, const dy_aug_row& r, int nsrc, int cx, int cy, float* v) {
  v[0] = v[1] = v[2] = 114.0f;
  if ((unsigned)cx >= (unsigned)r.cw || (unsigned)cy >= (unsigned)r.ch) return;
  const size_t plane = (size_t)p.hs * p.ws;
  for (int i = 0; i < nsrc; ++i) {
    const dy_aug_src& q = r.src[i];
    if (cx < q.x1a || cx >= q.x2a || cy < q.y1a || cy >= q.y2a) continue;
    const int sx = q.x1b + (cx - q.x1a), sy = q.y1b + (cy - q.y1a);
    // a row built wrongly (index / origin out of range) reads nothing: the rectangle shows 114
    if ((unsigned)q.index >= (unsigned)p.n || (unsigned)sx >= (unsigned)p.ws || (unsigned)sy >= (unsigned)p.hs) {
      v[0] = v[1] = v[2] = 114.0f;
      continue;
    }
    const uint8_t* s = p.src + (size_t)q.index * 3 * plane + (size_t)sy * p.ws + sx;
    v[0] = (float)s[0], v[1] = (float)s[plane], v[2] = (float)s[2 * plane];
  }
}

// RandomHSV on one rounded RGB pixel (values 0..255 as floats, integers): cv2's 8-bit HSV ranges, the reference's three look-up rules
__device__ __forceinline__ void hsv_px(const float* off, float* v) {
  const float r = v[0], g = v[1], b = v[2];
  const float vmax = fmaxf(r, fmaxf(g, b)), vmin = fminf(r, fminf(g, b));
  const float d = vmax - vmin;
  float h = 0.0f, sat = 0.0f;
  if (d > 0.0f) {
    // One division of two exact integers each (numerators < 2^24): a quotient that is a tie (x.5) in exact arithmetic is one in fp32 too, and
    // any other lies >= 1 / 510 from a tie, so the rounded H and S do not depend on the precision they are computed in.
    sat = rintf(255.0f * d / vmax);
    float num;  // 30 x (sector offset x d + difference): 60 degrees per sector, stored as degrees / 2
    if (vmax == r) num = 30.0f * (g - b);
    else if (vmax == g) num = 30.0f * (b - r) + 60.0f * d;
    else num = 30.0f * (r - g) + 120.0f * d;
    if (num < 0.0f) num += 180.0f * d;
    h = rintf(num / d);
    if (h >= 180.0f) h -= 180.0f;
  }
  // lut_hue = ((x + r0) % 180), lut_sat = clip(x + r1, 0, 255) with entry 0 kept 0, lut_val = clip(x + r2, 0, 255); .astype(uint8) truncates
  float h2 = fmodf(h + off[0], 180.0f);
  if (h2 < 0.0f) h2 += 180.0f;
  h2 = truncf(h2);
  if (h2 >= 180.0f) h2 = 0.0f;
  const float s2 = sat > 0.0f ? truncf(fminf(fmaxf(sat + off[1], 0.0f), 255.0f)) : 0.0f;
  const float v2 = truncf(fminf(fmaxf(vmax + off[2], 0.0f), 255.0f));
  // back: sector i of six, fraction f
  const int i = (int)h2 / 30;
  const float f = (h2 - 30.0f * (float)i) / 30.0f;
  const float s = s2 / 255.0f;
  const float pp = v2 * (1.0f - s), qq = v2 * (1.0f - s * f), tt = v2 * (1.0f - s * (1.0f - f));
  float ro, go, bo;
  switch (i) {
    case 0: ro = v2, go = tt, bo = pp; break;
    case 1: ro = qq, go = v2, bo = pp; break;
    case 2: ro = pp, go = v2, bo = tt; break;
    case 3: ro = pp, go = qq, bo = v2; break;
    case 4: ro = tt, go = pp, bo = v2; break;
    default: ro = v2, go = pp, bo = qq; break;
  }
  v[0] = fminf(fmaxf(rintf(ro), 0.0f), 255.0f);
  v[1] = fminf(fmaxf(rintf(go), 0.0f), 255.0f);
  v[2] = fminf(fmaxf(rintf(bo), 0.0f), 255.0f);
}

__global__ __launch_bounds__(256) void augment_kernel(const AugArgs p) {
  const int img = blockIdx.y;
  const dy_aug_row& r = p.table[img];  // wave-uniform: scalar loads
  const int quads = p.s >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= quads * p.s) return;
  const int y = t / quads, x0 = (t - y * quads) << 2;
  const int nsrc = (r.n_src == 1 || r.n_src == 4) ? r.n_src : 0;
  const int flags = r.flags;
  const int ys = (flags & DY_AUG_FLIPUD) ? p.s - 1 - y : y;
  uint32_t word[3] = {0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + k;
    const float xf = (float)((flags & DY_AUG_FLIPLR) ? p.s - 1 - x : x), yf = (float)ys;
    const float w = r.minv[6] * xf + r.minv[7] * yf + r.minv[8];
    const float u = (r.minv[0] * xf + r.minv[1] * yf + r.minv[2]) / w;
    const float v = (r.minv[3] * xf + r.minv[4] * yf + r.minv[5]) / w;
    float o[3] = {114.0f, 114.0f, 114.0f};
    // (negated comparisons: a NaN / infinite coordinate, e.g. w == 0, is "outside" too)
    if (u > -1.0f && v > -1.0f && u < (float)r.cw && v < (float)r.ch) {
      const float fu = floorf(u), fv = floorf(v);
      const int cx = (int)fu, cy = (int)fv;
      const float ax = u - fu, ay = v - fv;
      float v00[3], v01[3], v10[3], v11[3];
      canvas_px(p, r, nsrc, cx, cy, v00);
      canvas_px(p, r, nsrc, cx + 1, cy, v01);
      canvas_px(p, r, nsrc, cx, cy + 1, v10);
      canvas_px(p, r, nsrc, cx + 1, cy + 1, v11);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = v00[c] + ax * (v01[c] - v00[c]), bot = v10[c] + ax * (v11[c] - v10[c]);
        o[c] = rintf(top + ay * (bot - top));
      }
    }
    if (!(flags & DY_AUG_HSV_OFF)) hsv_px(r.hsv, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) word[c] |= (uint32_t)o[c] << (8 * k);
  }
  const size_t plane = (size_t)p.s * p.s;
  uint32_t* d = reinterpret_cast<uint32_t*>(p.dst + (size_t)img * 3 * plane + (size_t)y * p.s + x0);
  d[0] = word[0];
  d[plane >> 2] = word[1];
  d[plane >> 1] = word[2];
}

}  // namespace dy

extern "C" int32_t dy_augment_u8_nchw(const uint8_t* src, const dy_aug_row* table, uint8_t* dst, int32_t n_src_imgs, int32_t hs, int32_t ws, int32_t batch,
                                      int32_t s, dy_stream_t stream) {
  DY_REQUIRE(src && table && dst, DY_ERR_INVALID_ARG, "dy_augment_u8_nchw: null pointer");
  DY_REQUIRE(n_src_imgs > 0 && hs > 0 && ws > 0 && batch > 0 && s > 0, DY_ERR_INVALID_ARG, "dy_augment_u8_nchw: sizes must be positive");
  DY_REQUIRE(s % 4 == 0, DY_ERR_INVALID_ARG, "dy_augment_u8_nchw: s = %d must be a multiple of 4 (four pixels per 32-bit store)", s);
  DY_REQUIRE(((uintptr_t)dst & 3) == 0, DY_ERR_INVALID_ARG, "dy_augment_u8_nchw: dst must be 4-byte aligned");
  DY_REQUIRE(batch <= 65535 && s <= 16384, DY_ERR_INVALID_ARG, "dy_augment_u8_nchw: batch <= 65535 and s <= 16384");
  dy::AugArgs a{};
  a.src = src, a.table = table, a.dst = dst, a.n = n_src_imgs, a.hs = hs, a.ws = ws, a.batch = batch, a.s = s;
  const int threads = (s / 4) * s;
  hipLaunchKernelGGL(dy::augment_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)batch), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return dy::check_launch("dy_augment_u8_nchw");
}
