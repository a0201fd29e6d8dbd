// v8OBBLoss on the device: rotated TaskAlignedAssigner + BCE / ProbIoU / DFL losses, value and gradient.
// Reference: utils/loss.py:612-725 (v8OBBLoss), :116-137 (RotatedBboxLoss); utils/tal.py:298-330 (RotatedTaskAlignedAssigner) on top of
// :14-295 (TaskAlignedAssigner); :366-385 (dist2rbox); utils/metrics.py:178-241 (probiou).
//
// Same sparse shape as loss.hip (which this file leaves alone: dy_detection_loss stays the code it was), one kernel per stage:
//   L  obb_label_kernel     per label row [cls, x, y, w, h, r] (pixels, radians): mask_gt over all five numbers, the covariance row, the
//                           corners' edge vectors of the in-box test and the half extents of the axis-aligned hull -- once per label;
//   K1 obb_decode_kernel    per (image, anchor, side): DFL softmax expectation; the quad then shares (l, t, r, b): theta = (sigmoid(z) - 0.25) pi,
//                           dist2rbox, the pixel-unit covariance row of the prediction (kept for the assigner), dense softplus sum;
//   K2 obb_pick_kernel      one wave per label: the hull's cells per level, the reference's four inclusive inequalities, metric =
//                           s^alpha * ProbIoU^beta through probiou.h, top-k by wave arg-max rounds, claim counts;
//   K3 obb_resolve_kernel   per pick: shared anchors go to the largest overlap over ALL labels of the image (first index on ties);
//   K4 obb_gtmax_kernel     per foreground anchor: per-label maxima of metric and overlap;
//   K5 obb_fg_kernel        per foreground anchor: soft target, sums of t, x_cls t, (1 - ProbIoU_grid) t, DFL t.  ProbIoU is evaluated again
//                           in GRID units here, as the reference does (loss.py:697): not the assigner's pixel-unit value;
//   K6 obb_final_kernel     gains and total;
//   K7 obb_grad_dense_kernel / obb_grad_kernel   d total / d head maps and d total / d angle logit; the angle map is written whole.
// Deviation (as in loss.hip): a pick with metric exactly 0 is never taken.  Ties: equal metrics by ascending anchor index, equal overlaps
// by first label index.
#include "probiou.h"

#pragma clang fp contract(off)

namespace dy {

struct ObbLossArgs {
  const float* level[DY_MAX_LEVELS];
  const float* angle[DY_MAX_LEVELS];
  int h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS], lda[DY_MAX_LEVELS], a0[DY_MAX_LEVELS + 1];
  float stride[DY_MAX_LEVELS];
  int n_levels, batch, nc, A, gmax, topk;
  float alpha, beta, box_gain, cls_gain, dfl_gain;
  const float* gt;   // (batch, gmax, 6): cls, x, y, w, h (pixels), r (radians); rows with x+y+w+h+r <= 0 are padding
  float* lab;        // (batch, gmax, kLab): obb_label_kernel's row
  float* prow;       // (batch, A, 8): x, y, a, b, c of the predicted box in pixels (RRow), 3 floats of padding
  int* claims;       // (batch, A)
  int* owner;        // (batch, A) label index or -1
  int* picks;        // (batch, gmax, topk) anchor index or -1
  unsigned* gmax_al; // (batch, gmax) float bits
  unsigned* gmax_ov;
  double* acc;       // [0] sum softplus, [1] sum t, [2] sum x_cls t, [3] sum (1 - probiou) t, [4] sum dfl t, [5] n_fg
  float* out;        // [4]
  float* glevel[DY_MAX_LEVELS];
  float* gangle[DY_MAX_LEVELS];
  int gld[DY_MAX_LEVELS], glda[DY_MAX_LEVELS];
};

constexpr int kObbRegMax = 16;
constexpr int kLab = 20;
enum { LV = 0, LCLS, LX, LY, LA, LB, LC, LPX, LPY, LABX, LABY, LADX, LADY, LNAB, LNAD, LHX, LHY, LW, LH, LR };
constexpr float kPi = 3.14159265358979323846f;

__device__ __forceinline__ double obb_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// Sum over the 256-thread workgroup, in thread 0: ONE atomic per workgroup and value (loss.hip: per-wave atomics serialise)
__device__ __forceinline__ double obb_block_sum(double v, double* red /* [4] in LDS */) {
  v = obb_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ void obb_locate(const ObbLossArgs& p, int a, int* lvl, int* gx, int* gy) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < DY_MAX_LEVELS; ++i)
    if (i < p.n_levels && a >= p.a0[i]) l = i;
  const int al = a - p.a0[l];
  *lvl = l;
  *gy = al / p.w[l];
  *gx = al - *gy * p.w[l];
}

__device__ __forceinline__ float obb_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- L: one thread per label row ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void obb_label_kernel(const ObbLossArgs p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.batch * p.gmax) return;
  const float* g = p.gt + (size_t)i * 6;
  float* o = p.lab + (size_t)i * kLab;
  const float x = g[1], y = g[2], w = g[3], h = g[4], r = g[5];
  o[LV] = ((((x + y) + w) + h) + r) > 0.f ? 1.f : 0.f;  // mask_gt over all five numbers (loss.py:664)
  int c = (int)g[0];
  c = c < 0 ? 0 : (c >= p.nc ? p.nc - 1 : c);  // check_classes refuses such a table on the host; here it only must not read outside the row
  o[LCLS] = (float)c;
  const RRow rr = rnms_row(x, y, w, h, r);
  o[LX] = rr.x, o[LY] = rr.y, o[LA] = rr.a, o[LB] = rr.b, o[LC] = rr.c;
  // xywhr2xyxyxyxy (ops.py:589-600): pt1 = ctr + vec1 + vec2 (a), pt2 = ctr + vec1 - vec2 (b), pt4 = ctr - vec1 + vec2 (d)
  const float cs = cosf(r), sn = sinf(r);
  const float v1x = (w / 2.f) * cs, v1y = (w / 2.f) * sn, v2x = ((-h) / 2.f) * sn, v2y = (h / 2.f) * cs;
  const float ax = (x + v1x) + v2x, ay = (y + v1y) + v2y;
  const float bx = (x + v1x) - v2x, by = (y + v1y) - v2y;
  const float dx = (x - v1x) + v2x, dy_ = (y - v1y) + v2y;
  const float abx = bx - ax, aby = by - ay, adx = dx - ax, ady = dy_ - ay;
  o[LPX] = ax, o[LPY] = ay, o[LABX] = abx, o[LABY] = aby, o[LADX] = adx, o[LADY] = ady;
  o[LNAB] = abx * abx + aby * aby;
  o[LNAD] = adx * adx + ady * ady;
  o[LHX] = (fabsf(w * cs) + fabsf(h * sn)) * 0.5f;
  o[LHY] = (fabsf(w * sn) + fabsf(h * cs)) * 0.5f;
  o[LW] = w, o[LH] = h, o[LR] = r;
}

// ---- K1 ------------------------------------------------------------------------------------------------------------
// Thread = (anchor, side) as in loss_decode_kernel: the side's 16 bins are one 64-byte run.  The four lanes of an anchor then exchange
// their distances; lane 0 sums the class softplus terms, lane 1 builds the rotated box and its covariance row.
__global__ __launch_bounds__(256) void obb_decode_kernel(const ObbLossArgs p) {
  __shared__ double red[4];
  double sp = 0.0;
  const int lane = threadIdx.x & 63, q0 = lane & ~3;
  for (int l = 0; l < p.n_levels; ++l) {
    const unsigned w = (unsigned)p.w[l], hw = (unsigned)p.h[l] * w, total = (unsigned)p.batch * hw * 4u;  // a multiple of 4: quads stay whole
    const float* __restrict__ lv = p.level[l];
    const float* __restrict__ an = p.angle[l];
    const size_t ld = (size_t)p.ld[l], lda = (size_t)p.lda[l];
    const unsigned a0 = (unsigned)p.a0[l];
    const float st = p.stride[l];
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < total; t += gridDim.x * 256u) {
      const unsigned row = t >> 2;
      const int sd = (int)(t & 3);
      const unsigned b = row / hw, al = row - b * hw;
      const unsigned gy = al / w, gx = al - gy * w;
      const size_t idx = (size_t)b * p.A + a0 + al;
      const float* r = lv + (size_t)row * ld;
      float q[kObbRegMax];
      const float* src = r + sd * kObbRegMax;
      if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
#pragma unroll
        for (int i = 0; i < kObbRegMax; i += 4) {
          const float4 v = *reinterpret_cast<const float4*>(src + i);
          q[i] = v.x, q[i + 1] = v.y, q[i + 2] = v.z, q[i + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < kObbRegMax; ++i) q[i] = src[i];
      }
      float mx = q[0];
#pragma unroll
      for (int i = 1; i < kObbRegMax; ++i) mx = fmaxf(mx, q[i]);
      float den = 0.f, num = 0.f;
#pragma unroll
      for (int i = 0; i < kObbRegMax; ++i) {
        const float e = expf(q[i] - mx);
        den += e;
        num += e * (float)i;
      }
      const float d = num / den;
      const float dl = __shfl(d, q0), dt = __shfl(d, q0 + 1), dr = __shfl(d, q0 + 2), db = __shfl(d, q0 + 3);
      if (sd == 0) {
        const float* cl = r + 4 * kObbRegMax;
        float sm = 0.f;
        for (int c = 0; c < p.nc; ++c) {
          const float x = cl[c];
          sm += fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));  // BCEWithLogits against target 0
        }
        sp += (double)sm;
        p.claims[idx] = 0;
        p.owner[idx] = -1;
      } else if (sd == 1) {
        // head.py:222 angle = (sigmoid - 0.25) pi; tal.py:379-385 dist2rbox in grid units; loss.py:679 xywh times the stride
        const float th = (obb_sigmoid(an[(size_t)row * lda]) - 0.25f) * kPi;
        const float cs = cosf(th), sn = sinf(th);
        const float xf = (dr - dl) / 2.f, yf = (db - dt) / 2.f;
        const float x = ((xf * cs - yf * sn) + ((float)gx + 0.5f)) * st, y = ((xf * sn + yf * cs) + ((float)gy + 0.5f)) * st;
        const RRow rr = rnms_row(x, y, (dl + dr) * st, (dt + db) * st, th);
        float4* o = reinterpret_cast<float4*>(p.prow + idx * 8);  // the workspace is 256-byte aligned, rows are 32 bytes
        o[0] = float4{rr.x, rr.y, rr.a, rr.b};
        o[1] = float4{rr.c, 0.f, 0.f, 0.f};
      }
    }
  }
  sp = obb_block_sum(sp, red);
  if (threadIdx.x == 0 && sp != 0.0) atomicAdd(p.acc + 0, sp);
}

// metric and overlap of (label row lb of image b, anchor a); 0 when the anchor centre is outside the rotated rectangle (edges are inside)
__device__ __forceinline__ void obb_pair_metric(const ObbLossArgs& p, int b, const float* lb, int a, float* metric, float* overlap) {
  int l, gx, gy;
  obb_locate(p, a, &l, &gx, &gy);
  const float cx = ((float)gx + 0.5f) * p.stride[l], cy = ((float)gy + 0.5f) * p.stride[l];
  *metric = 0.f;
  *overlap = 0.f;
  // tal.py:325-330, in that order
  const float apx = cx - lb[LPX], apy = cy - lb[LPY];
  const float dab = apx * lb[LABX] + apy * lb[LABY];
  const float dad = apx * lb[LADX] + apy * lb[LADY];
  if (!((dab >= 0.f) && (dab <= lb[LNAB]) && (dad >= 0.f) && (dad <= lb[LNAD]))) return;
  const float* pr = p.prow + ((size_t)b * p.A + a) * 8;
  const RRow r1{lb[LX], lb[LY], lb[LA], lb[LB], lb[LC]}, r2{pr[0], pr[1], pr[2], pr[3], pr[4]};
  const float ov = fmaxf(rnms_probiou(r1, r2), 0.f);  // tal.py:303: probiou(gt, pred).clamp_(0)
  const float* row = p.level[l] + ((size_t)b * p.h[l] * p.w[l] + (a - p.a0[l])) * (size_t)p.ld[l];
  const float sc = obb_sigmoid(row[4 * kObbRegMax + (int)lb[LCLS]]);
  *overlap = ov;
  *metric = powf(sc, p.alpha) * powf(ov, p.beta);
}

// ---- K2: one wave per label --------------------------------------------------------------------------------------
// The hull's cells of every level are this label's candidates.  Their metrics are computed ONCE into LDS (up to kPickCache candidates: a
// 140 px rectangle on the P2 grid) and the top-k rounds scan that table, instead of evaluating every candidate again in every round as
// tal_pick_kernel does with its cheaper CIoU pairs: 1.03 -> 0.96 ms for 3,256 labels at B = 64 (tal_pick_kernel: 0.29 ms; what remains is
// four dependent passes per wave, the widened hull has candidates on every level: DESIGN section 22).  A larger hull falls back to
// re-evaluation: the same function on the same inputs, so both paths pick the same anchors.
constexpr int kPickCache = 1024;

struct PickHull {
  int gx0, gy0, nx, ny;
};
__device__ __forceinline__ PickHull obb_hull(const ObbLossArgs& p, const float* lb, int l) {
  const float st = p.stride[l];
  const float fw = (float)p.w[l], fh = (float)p.h[l];
  // one cell wider on every side; the floats are clamped to the map BEFORE the conversion (a label may be anywhere, or NaN)
  const float fx0 = fminf(fmaxf(floorf((lb[LX] - lb[LHX]) / st - 0.5f) - 1.f, 0.f), fw);
  const float fx1 = fminf(fmaxf(ceilf((lb[LX] + lb[LHX]) / st - 0.5f) + 1.f, -1.f), fw - 1.f);
  const float fy0 = fminf(fmaxf(floorf((lb[LY] - lb[LHY]) / st - 0.5f) - 1.f, 0.f), fh);
  const float fy1 = fminf(fmaxf(ceilf((lb[LY] + lb[LHY]) / st - 0.5f) + 1.f, -1.f), fh - 1.f);
  if (!(fx1 >= fx0 && fy1 >= fy0)) return PickHull{0, 0, 0, 0};
  return PickHull{(int)fx0, (int)fy0, (int)fx1 - (int)fx0 + 1, (int)fy1 - (int)fy0 + 1};
}

__global__ __launch_bounds__(64) void obb_pick_kernel(const ObbLossArgs p) {
  __shared__ float s_m[kPickCache];
  __shared__ int s_a[kPickCache];
  const int bg = blockIdx.x, b = bg / p.gmax, lane = threadIdx.x;
  const float* lb = p.lab + (size_t)bg * kLab;
  int* picks = p.picks + (size_t)bg * p.topk;
  for (int k = lane; k < p.topk; k += 64) picks[k] = -1;
  if (!(lb[LV] > 0.f)) return;
  int total = 0;  // wave-uniform
  for (int l = 0; l < p.n_levels; ++l) {
    const PickHull hl = obb_hull(p, lb, l);
    const int n = hl.nx * hl.ny;
    if (total + n <= kPickCache) {
      for (int i = lane; i < n; i += 64) {
        const int a = p.a0[l] + (hl.gy0 + i / hl.nx) * p.w[l] + hl.gx0 + i % hl.nx;
        float m, ov;
        obb_pair_metric(p, b, lb, a, &m, &ov);
        s_m[total + i] = m;
        s_a[total + i] = a;
      }
    }
    total += n;
  }
  const bool cached = total <= kPickCache;
  __syncthreads();
  float last_m = 3.0e38f;
  int last_a = -1;  // picks proceed in (metric desc, anchor asc) order; ties resolved by anchor index
  for (int k = 0; k < p.topk; ++k) {
    float bm = 0.f;
    int ba = 0x7fffffff;
    // candidates strictly after the previous pick in (metric desc, anchor asc) order; a metric of exactly 0 is never taken
    auto consider = [&](float m, int a) {
      const bool after = (m < last_m) || (m == last_m && a > last_a);
      if (m > 0.f && after && (m > bm || (m == bm && a < ba))) {
        bm = m;
        ba = a;
      }
    };
    if (cached) {
      for (int i = lane; i < total; i += 64) consider(s_m[i], s_a[i]);
    } else {
      for (int l = 0; l < p.n_levels; ++l) {
        const PickHull hl = obb_hull(p, lb, l);
        for (int i = lane; i < hl.nx * hl.ny; i += 64) {
          const int a = p.a0[l] + (hl.gy0 + i / hl.nx) * p.w[l] + hl.gx0 + i % hl.nx;
          float m, ov;
          obb_pair_metric(p, b, lb, a, &m, &ov);
          consider(m, a);
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(bm, o);
      const int oa = __shfl_xor(ba, o);
      if (om > bm || (om == bm && oa < ba)) {
        bm = om;
        ba = oa;
      }
    }
    if (!(bm > 0.f)) break;
    if (lane == 0) {
      picks[k] = ba;
      atomicAdd(p.claims + (size_t)b * p.A + ba, 1);
    }
    last_m = bm;
    last_a = ba;
  }
}

// ---- K3: one thread per pick ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void obb_resolve_kernel(const ObbLossArgs p) {
  const long long total = (long long)p.batch * p.gmax * p.topk;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int a = p.picks[idx];
    if (a < 0) continue;
    const int bg = (int)(idx / p.topk), b = bg / p.gmax, g = bg - b * p.gmax;
    int own = g;
    if (p.claims[(size_t)b * p.A + a] > 1) {  // tal.py:281-288
      float best = -1.f;
      for (int gg = 0; gg < p.gmax; ++gg) {
        const float* lb = p.lab + ((size_t)b * p.gmax + gg) * kLab;
        float m = 0.f, ov = 0.f;
        if (lb[LV] > 0.f) obb_pair_metric(p, b, lb, a, &m, &ov);
        if (ov > best) {
          best = ov;
          own = gg;
        }
      }
    }
    p.owner[(size_t)b * p.A + a] = own;
  }
}

// ---- K4 ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void obb_gtmax_kernel(const ObbLossArgs p) {
  const long long total = (long long)p.batch * p.A;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int g = p.owner[idx];
    if (g < 0) continue;
    const int b = (int)(idx / p.A), a = (int)(idx - (long long)b * p.A);
    float m, ov;
    obb_pair_metric(p, b, p.lab + ((size_t)b * p.gmax + g) * kLab, a, &m, &ov);
    atomicMax(p.gmax_al + (size_t)b * p.gmax + g, __float_as_uint(m));
    atomicMax(p.gmax_ov + (size_t)b * p.gmax + g, __float_as_uint(ov));
  }
}

// Forward-mode dual over the five inputs of a foreground anchor's box: (l, t, r, b) in grid units and the angle theta.
struct D5 {
  float v, g[5];
};
__device__ __forceinline__ D5 d5c(float c) { return D5{c, {0.f, 0.f, 0.f, 0.f, 0.f}}; }
__device__ __forceinline__ D5 d5var(float c, int i) {
  D5 r = d5c(c);
  r.g[i] = 1.f;
  return r;
}
#define D5_EACH(expr)            \
  D5 r;                          \
  _Pragma("unroll") for (int i = 0; i < 5; ++i) r.g[i] = (expr);
__device__ __forceinline__ D5 operator+(D5 a, D5 b) {
  D5_EACH(a.g[i] + b.g[i]);
  r.v = a.v + b.v;
  return r;
}
__device__ __forceinline__ D5 operator-(D5 a, D5 b) {
  D5_EACH(a.g[i] - b.g[i]);
  r.v = a.v - b.v;
  return r;
}
__device__ __forceinline__ D5 operator*(D5 a, D5 b) {
  D5_EACH(a.g[i] * b.v + a.v * b.g[i]);
  r.v = a.v * b.v;
  return r;
}
__device__ __forceinline__ D5 operator/(D5 a, D5 b) {
  const float q = a.v / b.v, ib = 1.f / b.v;
  D5_EACH((a.g[i] - q * b.g[i]) * ib);
  r.v = q;
  return r;
}
__device__ __forceinline__ D5 d5chain(D5 a, float v, float dv) {  // f(a) with f(a.v) = v and f'(a.v) = dv
  D5_EACH(a.g[i] * dv);
  r.v = v;
  return r;
}
__device__ __forceinline__ D5 d5scale(D5 a, float c) { return d5chain(a, a.v * c, c); }
__device__ __forceinline__ D5 d5clamp(D5 a, float lo, float hi) { return a.v < lo ? d5c(lo) : (a.v > hi ? d5c(hi) : a); }  // gradient inside [lo, hi], ends included, as torch.clamp
__device__ __forceinline__ D5 d5min0(D5 a) { return a.v < 0.f ? d5c(0.f) : a; }                                          // clamp_(0)

struct Cov5 {
  D5 a, b, c;
};
// _get_covariance_matrix (metrics.py:189-195) of a dual box
__device__ __forceinline__ Cov5 cov5(D5 w, D5 h, D5 cs, D5 sn) {
  const D5 a = d5scale(w * w, 1.f / 12.f), b = d5scale(h * h, 1.f / 12.f);
  const D5 cs2 = cs * cs, sn2 = sn * sn;
  return Cov5{a * cs2 + b * sn2, a * sn2 + b * cs2, ((a - b) * cs) * sn};
}

// probiou(obb1 = prediction, obb2 = target) (metrics.py:217-233) with its derivative w.r.t. the prediction's (l, t, r, b, theta); the value
// follows rnms_probiou term for term (box 1 = prediction), the derivative passes the three clamps as autograd does.
__device__ __forceinline__ D5 probiou_dual(D5 x1, D5 y1, const Cov5& c1, const RRow& r2) {
  const float eps = 1e-7f;
  const D5 sa = c1.a + d5c(r2.a), sb = c1.b + d5c(r2.b), sc = c1.c + d5c(r2.c);
  const D5 dy_ = y1 - d5c(r2.y), dx = x1 - d5c(r2.x);
  const D5 det = sa * sb - sc * sc;
  const D5 den = det + d5c(eps);
  const D5 t1 = d5scale((sa * (dy_ * dy_) + sb * (dx * dx)) / den, 0.25f);
  const D5 t2 = d5scale(((sc * (d5c(r2.x) - x1)) * dy_) / den, 0.5f);
  const D5 d1 = d5min0(c1.a * c1.b - c1.c * c1.c);
  float d2 = r2.a * r2.b - r2.c * r2.c;
  d2 = d2 < 0.f ? 0.f : d2;
  const D5 pr = d5scale(d1, d2);
  const float sq = sqrtf(pr.v);
  const D5 root = d5chain(pr, sq, 0.5f / sq);
  const D5 arg = det / (d5scale(root, 4.f) + d5c(eps)) + d5c(eps);
  const D5 t3 = d5scale(d5chain(arg, logf(arg.v), 1.f / arg.v), 0.5f);
  const D5 bd = d5clamp((t1 + t2) + t3, eps, 100.f);
  const float ex = expf(-bd.v);
  const D5 in = d5chain(bd, (1.f - ex) + eps, ex);
  const float hd = sqrtf(in.v);
  const D5 h = d5chain(in, hd, 0.5f / hd);
  return d5c(1.f) - h;
}

// What K5 and K7 share for one foreground anchor: soft target, softmax of the four sides, the grid-unit box loss with its derivative, DFL
struct FgRow {
  float t, x_cls, box, dfl;
  int tc;
};

template <bool GRAD>
__device__ __forceinline__ FgRow obb_fg_row(const ObbLossArgs& p, long long idx, int g, float* go, float* ga, float inv) {
  const int b = (int)(idx / p.A), a = (int)(idx - (long long)b * p.A);
  const float* lb = p.lab + ((size_t)b * p.gmax + g) * kLab;
  float m, ov;
  obb_pair_metric(p, b, lb, a, &m, &ov);
  const float pal = __uint_as_float(p.gmax_al[(size_t)b * p.gmax + g]), pov = __uint_as_float(p.gmax_ov[(size_t)b * p.gmax + g]);
  FgRow o;
  o.t = m * pov / (pal + 1e-9f);  // tal.py:111-116
  o.tc = (int)lb[LCLS];
  int l, gx, gy;
  obb_locate(p, a, &l, &gx, &gy);
  const size_t row = (size_t)b * p.h[l] * p.w[l] + (a - p.a0[l]);
  const float* r = p.level[l] + row * (size_t)p.ld[l];
  o.x_cls = r[4 * kObbRegMax + o.tc];
  const float st = p.stride[l];
  const float ax = (float)gx + 0.5f, ay = (float)gy + 0.5f;
  float pr[4][kObbRegMax], d[4], lse[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float* q = r + s * kObbRegMax;
    float mx = q[0];
    for (int i = 1; i < kObbRegMax; ++i) mx = fmaxf(mx, q[i]);
    float den = 0.f;
    for (int i = 0; i < kObbRegMax; ++i) {
      pr[s][i] = expf(q[i] - mx);
      den += pr[s][i];
    }
    float num = 0.f;
    for (int i = 0; i < kObbRegMax; ++i) {
      pr[s][i] /= den;
      num += pr[s][i] * (float)i;
    }
    d[s] = num;
    lse[s] = mx + logf(den);
  }
  const float z = p.angle[l][row * (size_t)p.lda[l]];
  const float sg = obb_sigmoid(z);
  const float th = (sg - 0.25f) * kPi;
  // dist2rbox (tal.py:379-385) on duals: inputs 0..3 = l, t, r, b, input 4 = theta
  const D5 dl = d5var(d[0], 0), dt = d5var(d[1], 1), dr = d5var(d[2], 2), db = d5var(d[3], 3);
  const D5 cs = d5chain(d5var(th, 4), cosf(th), -sinf(th)), sn = d5chain(d5var(th, 4), sinf(th), cosf(th));
  const D5 xf = d5scale(dr - dl, 0.5f), yf = d5scale(db - dt, 0.5f);
  const D5 x = (xf * cs - yf * sn) + d5c(ax), y = (xf * sn + yf * cs) + d5c(ay);
  const Cov5 c1 = cov5(dl + dr, dt + db, cs, sn);
  // target / stride (loss.py:697): grid units, the angle unscaled
  const float tx = lb[LX] / st, ty = lb[LY] / st, tw = lb[LW] / st, thh = lb[LH] / st;
  const RRow r2 = rnms_row(tx, ty, tw, thh, lb[LR]);
  const D5 iou = probiou_dual(x, y, c1, r2);
  o.box = 1.f - iou.v;
  // DFL target (loss.py:131): the UNROTATED box of the target's xywh
  const float x1 = tx - tw / 2.f, y1 = ty - thh / 2.f, x2 = tx + tw / 2.f, y2 = ty + thh / 2.f;
  const float tgt[4] = {ax - x1, ay - y1, x2 - ax, y2 - ay};
  float dfl = 0.f;
  const float kb = -o.t * p.box_gain * inv;  // d total / d probiou
  const float kd = o.t * p.dfl_gain * inv * 0.25f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float tv = fminf(fmaxf(tgt[s], 0.f), (float)(kObbRegMax - 1) - 0.01f);
    const int tl = (int)tv;
    const float wl = (float)(tl + 1) - tv, wr = 1.f - wl;
    const float* q = r + s * kObbRegMax;
    dfl += (lse[s] - q[tl]) * wl + (lse[s] - q[tl + 1]) * wr;
    if constexpr (GRAD) {
      const float gd = iou.g[s] * kb;
      for (int i = 0; i < kObbRegMax; ++i) {
        const float onehot = (i == tl ? wl : 0.f) + (i == tl + 1 ? wr : 0.f);
        go[s * kObbRegMax + i] = gd * pr[s][i] * ((float)i - d[s]) + kd * (pr[s][i] - onehot);
      }
    }
  }
  o.dfl = dfl * 0.25f;
  if constexpr (GRAD) *ga = (iou.g[4] * kb) * (kPi * (sg * (1.f - sg)));  // through theta = (sigmoid(z) - 0.25) pi
  return o;
}

// ---- K5 ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void obb_fg_kernel(const ObbLossArgs p) {
  __shared__ double red[4];
  const long long total = (long long)p.batch * p.A;
  double s_t = 0.0, s_xt = 0.0, s_box = 0.0, s_dfl = 0.0, s_n = 0.0;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int g = p.owner[idx];
    if (g < 0) continue;
    const FgRow f = obb_fg_row<false>(p, idx, g, nullptr, nullptr, 0.f);
    s_t += (double)f.t;
    s_xt += (double)(f.x_cls * f.t);
    s_box += (double)(f.box * f.t);
    s_dfl += (double)(f.dfl * f.t);
    s_n += 1.0;
  }
  s_t = obb_block_sum(s_t, red), s_xt = obb_block_sum(s_xt, red), s_box = obb_block_sum(s_box, red), s_dfl = obb_block_sum(s_dfl, red),
  s_n = obb_block_sum(s_n, red);
  if (threadIdx.x == 0 && s_n != 0.0) {
    atomicAdd(p.acc + 1, s_t);
    atomicAdd(p.acc + 2, s_xt);
    atomicAdd(p.acc + 3, s_box);
    atomicAdd(p.acc + 4, s_dfl);
    atomicAdd(p.acc + 5, s_n);
  }
}

// ---- K7 ------------------------------------------------------------------------------------------------------------
// DENSE: thread = one 16-byte chunk of a BACKGROUND anchor's gradient row (loss_grad_dense_kernel's scheme: zeros in the box bins,
// sigmoid(x) * gain in the class slots, rows with less than 8 floats of padding written whole); the thread of chunk 0 also writes the
// anchor's WHOLE angle-gradient row as zeros.  SPARSE: thread = foreground anchor.  Together they rewrite both maps completely each call.
__global__ __launch_bounds__(256) void obb_grad_dense_kernel(const ObbLossArgs p, unsigned chunks_values) {
  const double tss_d = p.acc[1] > 1.0 ? p.acc[1] : 1.0;
  const float inv = (float)((double)p.batch / tss_d);
  for (int l = 0; l < p.n_levels; ++l) {  // level by level: per-level arguments stay scalars
    const unsigned hw = (unsigned)(p.h[l] * p.w[l]);
    const float* __restrict__ lv = p.level[l];
    float* __restrict__ gl = p.glevel[l];
    float* __restrict__ ga = p.gangle[l];
    const size_t ld = (size_t)p.ld[l], gld = (size_t)p.gld[l];
    const int glda = p.glda[l];
    const unsigned a0 = (unsigned)p.a0[l];
    const int nval = 4 * kObbRegMax + p.nc;
    const bool whole = gld % 4 == 0 && (int)gld - nval < 8;
    const unsigned chunks = whole ? (unsigned)(gld / 4) : chunks_values;
    const int lim = whole ? (int)gld : nval;
    const unsigned total = (unsigned)p.batch * hw * chunks;
    for (unsigned tt = blockIdx.x * 256u + threadIdx.x; tt < total; tt += gridDim.x * 256u) {
      const unsigned row = tt / chunks;
      const int ch = (int)(tt - row * chunks);
      const unsigned b = row / hw, al = row - b * hw;
      if (p.owner[(size_t)b * p.A + a0 + al] >= 0) continue;  // the sparse launch writes both rows
      float* go = gl + (size_t)row * gld;
      if (ch == 0) {
        float* gr = ga + (size_t)row * glda;
        for (int j = 0; j < glda; ++j) gr[j] = 0.f;
      }
      if (ch < kObbRegMax) {
        float* gs = go + ch * 4;
        if ((reinterpret_cast<uintptr_t>(gs) & 15) == 0) *reinterpret_cast<float4*>(gs) = float4{0.f, 0.f, 0.f, 0.f};
        else gs[0] = 0.f, gs[1] = 0.f, gs[2] = 0.f, gs[3] = 0.f;
      } else {
        const int c0 = (ch - kObbRegMax) * 4;
        const float* cl = lv + (size_t)row * ld + 4 * kObbRegMax;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c0 + j < p.nc ? obb_sigmoid(cl[c0 + j]) * p.cls_gain * inv : 0.f;
        float* gs = go + 4 * kObbRegMax + c0;
        if (4 * kObbRegMax + c0 + 4 <= lim && (reinterpret_cast<uintptr_t>(gs) & 15) == 0) {
          *reinterpret_cast<float4*>(gs) = float4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * kObbRegMax + c0 + j < lim) gs[j] = v[j];
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void obb_grad_kernel(const ObbLossArgs p) {
  const long long total = (long long)p.batch * p.A;
  const double tss_d = p.acc[1] > 1.0 ? p.acc[1] : 1.0;
  const float inv = (float)((double)p.batch / tss_d);
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int g = p.owner[idx];
    if (g < 0) continue;
    const int b = (int)(idx / p.A), a = (int)(idx - (long long)b * p.A);
    int l, gx, gy;
    obb_locate(p, a, &l, &gx, &gy);
    const size_t row = (size_t)b * p.h[l] * p.w[l] + (a - p.a0[l]);
    float* go = p.glevel[l] + row * (size_t)p.gld[l];
    float* gr = p.gangle[l] + row * (size_t)p.glda[l];
    float gz;
    const FgRow f = obb_fg_row<true>(p, idx, g, go, &gz, inv);
    gr[0] = gz;
    for (int j = 1; j < p.glda[l]; ++j) gr[j] = 0.f;
    const float* cl = p.level[l] + row * (size_t)p.ld[l] + 4 * kObbRegMax;
    for (int c = 0; c < p.nc; ++c) go[4 * kObbRegMax + c] = (obb_sigmoid(cl[c]) - (c == f.tc ? f.t : 0.f)) * p.cls_gain * inv;
    const int nval = 4 * kObbRegMax + p.nc;
    if (p.gld[l] % 4 == 0 && p.gld[l] - nval < 8)  // the dense launch writes such rows whole: so does this one
      for (int j = nval; j < p.gld[l]; ++j) go[j] = 0.f;
  }
}

__global__ void obb_final_kernel(const ObbLossArgs p) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double tss = p.acc[1] > 1.0 ? p.acc[1] : 1.0;  // loss.py:689
  const double cls = (p.acc[0] - p.acc[2]) / tss;
  const double box = p.acc[5] > 0.0 ? p.acc[3] / tss : 0.0;
  const double dfl = p.acc[5] > 0.0 ? p.acc[4] / tss : 0.0;
  p.out[0] = (float)(box * p.box_gain);
  p.out[1] = (float)(cls * p.cls_gain);
  p.out[2] = (float)(dfl * p.dfl_gain);
  p.out[3] = (float)((box * p.box_gain + cls * p.cls_gain + dfl * p.dfl_gain) * p.batch);
}

// d total / d angle logit (fp32, channel 0 of a row of pitch ld_g) -> the angle tail's dz in the storage type: kObbAngleCout channels per row, the
// value times *scale (the deferred seed of the backward pass, or none) in channel 0 and zeros behind it -- the width the 1x1 kernels serve.
constexpr int kObbAngleCout = 8;
template <typename T>
__global__ __launch_bounds__(256) void obb_angle_grad_cast_kernel(const float* __restrict__ g, int ld_g, long long rows, const float* __restrict__ scale, T* __restrict__ dz,
                                                                   int ld_dz) {
  const float s = scale ? *scale : 1.f;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
    T* o = dz + r * ld_dz;
    o[0] = Elem<T>::from_f32(g[r * ld_g] * s);
#pragma unroll
    for (int j = 1; j < kObbAngleCout; ++j) o[j] = Elem<T>::from_f32(0.f);
  }
}

static inline size_t oalign(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace dy

using namespace dy;

extern "C" int64_t dy_obb_loss_workspace_bytes(int32_t batch, int32_t anchors, int32_t gmax, int32_t topk) {
  if (batch <= 0 || anchors <= 0 || gmax < 0 || topk <= 0) return -1;
  const size_t ba = (size_t)batch * anchors, bg = (size_t)batch * (gmax > 0 ? gmax : 1);
  return (int64_t)(oalign(ba * 32) + 2 * oalign(ba * 4) + oalign(bg * topk * 4) + oalign(bg * kLab * 4) + 2 * oalign(bg * 4) + oalign(6 * 8));
}

extern "C" int32_t dy_obb_loss(const dy_obb_loss_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->out && d->workspace, DY_ERR_INVALID_ARG, "dy_obb_loss: null pointer");
  DY_REQUIRE(d->n_levels >= 1 && d->n_levels <= DY_MAX_LEVELS && d->batch > 0 && d->nc > 0 && d->gmax >= 0 && d->topk > 0, DY_ERR_INVALID_ARG,
             "dy_obb_loss: bad dims");
  DY_REQUIRE(d->reg_max == kObbRegMax, DY_ERR_UNSUPPORTED, "dy_obb_loss: reg_max %d not built (only 16)", d->reg_max);
  DY_REQUIRE(d->gmax == 0 || d->gt, DY_ERR_INVALID_ARG, "dy_obb_loss: gt is null");
  ObbLossArgs a{};
  long long A = 0;
  for (int i = 0; i < d->n_levels; ++i) {
    DY_REQUIRE(d->level[i] && d->angle[i] && d->h[i] > 0 && d->w[i] > 0 && d->ld[i] >= 4 * d->reg_max + d->nc && d->ld_angle[i] >= 1, DY_ERR_INVALID_ARG,
               "dy_obb_loss: level %d invalid", i);
    a.level[i] = d->level[i];
    a.angle[i] = d->angle[i];
    a.h[i] = d->h[i];
    a.w[i] = d->w[i];
    a.ld[i] = d->ld[i];
    a.lda[i] = d->ld_angle[i];
    a.stride[i] = d->stride[i];
    DY_REQUIRE(d->stride[i] > 0.f, DY_ERR_INVALID_ARG, "dy_obb_loss: stride of level %d is not positive", i);
    a.a0[i] = (int)A;
    A += (long long)d->h[i] * d->w[i];
    DY_REQUIRE(A * d->batch < (1ll << 29), DY_ERR_UNSUPPORTED, "dy_obb_loss: too many anchors for 32-bit indices");
  }
  a.a0[d->n_levels] = (int)A;
  a.n_levels = d->n_levels;
  a.batch = d->batch;
  a.nc = d->nc;
  a.A = (int)A;
  a.gmax = d->gmax;
  a.topk = d->topk;
  a.alpha = d->alpha;
  a.beta = d->beta;
  a.box_gain = d->box_gain;
  a.cls_gain = d->cls_gain;
  a.dfl_gain = d->dfl_gain;
  a.gt = d->gt;
  a.out = d->out;
  const int64_t need = dy_obb_loss_workspace_bytes(d->batch, (int)A, d->gmax, d->topk);
  DY_REQUIRE(d->workspace_bytes >= need && aligned16(d->workspace), DY_ERR_WORKSPACE, "dy_obb_loss: workspace %lld < %lld bytes", (long long)d->workspace_bytes,
             (long long)need);
  unsigned char* ws = reinterpret_cast<unsigned char*>(d->workspace);
  const size_t ba = (size_t)d->batch * A, bg = (size_t)d->batch * (d->gmax > 0 ? d->gmax : 1);
  a.prow = reinterpret_cast<float*>(ws);
  ws += oalign(ba * 32);
  a.claims = reinterpret_cast<int*>(ws);
  ws += oalign(ba * 4);
  a.owner = reinterpret_cast<int*>(ws);
  ws += oalign(ba * 4);
  a.picks = reinterpret_cast<int*>(ws);
  ws += oalign(bg * d->topk * 4);
  a.lab = reinterpret_cast<float*>(ws);
  ws += oalign(bg * kLab * 4);
  a.gmax_al = reinterpret_cast<unsigned*>(ws);
  ws += oalign(bg * 4);
  a.gmax_ov = reinterpret_cast<unsigned*>(ws);
  ws += oalign(bg * 4);
  a.acc = reinterpret_cast<double*>(ws);
  const bool want_grad = d->grad_level[0] != nullptr;
  if (want_grad) {
    for (int i = 0; i < d->n_levels; ++i) {
      DY_REQUIRE(d->grad_level[i] && d->ld_grad[i] >= 4 * d->reg_max + d->nc && d->grad_angle[i] && d->ld_grad_angle[i] >= 1 && d->ld_grad_angle[i] <= 64,
                 DY_ERR_INVALID_ARG, "dy_obb_loss: grad level %d invalid", i);
      a.glevel[i] = d->grad_level[i];
      a.gld[i] = d->ld_grad[i];
      a.gangle[i] = d->grad_angle[i];
      a.glda[i] = d->ld_grad_angle[i];
    }
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  zero_async(a.gmax_al, 2 * oalign(bg * 4) + oalign(6 * 8), st);  // per-label maxima and accumulators: the contiguous tail; a kernel, never a memset node
  const long long tot = (long long)d->batch * A;
  const unsigned blocks = (unsigned)((tot + 255) / 256 < 4096 ? (tot + 255) / 256 : 4096);
  const unsigned blocks4 = (unsigned)((tot * 4 + 255) / 256 < 8192 ? (tot * 4 + 255) / 256 : 8192);
  if (d->gmax > 0) hipLaunchKernelGGL(obb_label_kernel, dim3((unsigned)((d->batch * d->gmax + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(obb_decode_kernel, dim3(blocks4), dim3(256), 0, st, a);
  if (d->gmax > 0) {
    hipLaunchKernelGGL(obb_pick_kernel, dim3((unsigned)(d->batch * d->gmax)), dim3(64), 0, st, a);
    const long long np = (long long)d->batch * d->gmax * d->topk;
    hipLaunchKernelGGL(obb_resolve_kernel, dim3((unsigned)((np + 255) / 256 < 4096 ? (np + 255) / 256 : 4096)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(obb_gtmax_kernel, dim3(blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(obb_fg_kernel, dim3(blocks), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(obb_final_kernel, dim3(1), dim3(64), 0, st, a);
  if (want_grad) {
    const unsigned chunks = (unsigned)(kObbRegMax + (d->nc + 3) / 4);
    DY_REQUIRE(tot * (chunks + 2) < (1ll << 32), DY_ERR_UNSUPPORTED, "dy_obb_loss: gradient map too large for 32-bit chunk indices");
    const long long nb = (tot * (chunks + 2) + 255) / 256;
    hipLaunchKernelGGL(obb_grad_dense_kernel, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, st, a, chunks);
    if (d->gmax > 0) hipLaunchKernelGGL(obb_grad_kernel, dim3(blocks), dim3(256), 0, st, a);
  }
  if (d->out_owner) {
    if (hipMemcpyAsync(d->out_owner, a.owner, ba * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return check_launch("dy_obb_loss copy");
  }
  return check_launch("dy_obb_loss");
}

extern "C" int32_t dy_obb_angle_grad_cast(const float* g, int32_t ld_g, int64_t rows, const float* scale, void* dz, int32_t ld_dz, int32_t dtype, dy_stream_t stream) {
  const int es = dtype_size_no_fp8(dtype);
  DY_REQUIRE(g && dz && rows > 0 && ld_g >= 1 && (es == 2 || es == 4), DY_ERR_INVALID_ARG, "dy_obb_angle_grad_cast: bad arguments");
  DY_REQUIRE(ld_dz >= kObbAngleCout && aligned16(dz) && (ld_dz * es) % 16 == 0, DY_ERR_INVALID_ARG, "dy_obb_angle_grad_cast: dz rows must hold %d channels in whole 16-byte chunks",
             kObbAngleCout);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = (unsigned)((rows + 255) / 256 < 4096 ? (rows + 255) / 256 : 4096);
  if (dtype == DY_BF16) hipLaunchKernelGGL((obb_angle_grad_cast_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, g, ld_g, (long long)rows, scale, (bf16_t*)dz, ld_dz);
  else if (dtype == DY_F16) hipLaunchKernelGGL((obb_angle_grad_cast_kernel<f16_t>), dim3(grid), dim3(256), 0, st, g, ld_g, (long long)rows, scale, (f16_t*)dz, ld_dz);
  else hipLaunchKernelGGL((obb_angle_grad_cast_kernel<float>), dim3(grid), dim3(256), 0, st, g, ld_g, (long long)rows, scale, (float*)dz, ld_dz);
  return check_launch("dy_obb_angle_grad_cast");
}
