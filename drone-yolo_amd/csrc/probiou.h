// ProbIoU of two oriented boxes, shared by the rotated NMS (obb.hip) and the validator's rotated matching (val_match.hip, the VmRotated policy): one
// expression, so a pair scores the same in both.  fp32 in the reference's order of operations; the including file keeps
// `#pragma clang fp contract(off)` in force (the pragma below covers this header's functions wherever it is included).
#pragma once
#include "common_hip.h"

#pragma clang fp contract(off)

namespace dy {

struct RRow {
  float x, y, a, b, c;
};

// _get_covariance_matrix (metrics.py:178-195) of one box
__device__ __forceinline__ RRow rnms_row(float x, float y, float w, float h, float th) {
  const float a = (w * w) / 12.f, b = (h * h) / 12.f;
  const float cs = cosf(th), sn = sinf(th);
  const float cs2 = cs * cs, sn2 = sn * sn;
  return RRow{x, y, a * cs2 + b * sn2, a * sn2 + b * cs2, ((a - b) * cs) * sn};
}

// batch_probiou(obb1 = r1, obb2 = r2) (metrics.py:259-275), term for term; the clamps keep a NaN as torch's do
__device__ __forceinline__ float rnms_probiou(const RRow& r1, const RRow& r2) {
  const float eps = 1e-7f;
  const float sa = r1.a + r2.a, sb = r1.b + r2.b, sc = r1.c + r2.c;
  const float dy = r1.y - r2.y, dx = r1.x - r2.x;
  const float det = sa * sb - sc * sc;
  const float den = det + eps;
  const float t1 = ((sa * (dy * dy) + sb * (dx * dx)) / den) * 0.25f;
  const float t2 = (((sc * (r2.x - r1.x)) * dy) / den) * 0.5f;
  float d1 = r1.a * r1.b - r1.c * r1.c, d2 = r2.a * r2.b - r2.c * r2.c;
  d1 = d1 < 0.f ? 0.f : d1;
  d2 = d2 < 0.f ? 0.f : d2;
  const float t3 = logf(det / (4.f * sqrtf(d1 * d2) + eps) + eps) * 0.5f;
  float bd = (t1 + t2) + t3;
  bd = bd < eps ? eps : (bd > 100.f ? 100.f : bd);
  const float hd = sqrtf((1.f - expf(-bd)) + eps);
  return 1.f - hd;
}

}  // namespace dy
