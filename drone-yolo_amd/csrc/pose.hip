// Pose estimation behind the Detect kernels: the prediction half of the reference's `pose` task, and the batched person-crop slicer.
//
//   dy_kpt_decode     Pose.kpts_decode (nn/modules/head.py:274-279, the non-export branch).  kpt_one() holds the arithmetic of one keypoint
//                     of one anchor; two kernels call it:
//                       dense   pred_kpt (batch, nk, anchors) for the module-level return: thread = (image, keypoint, anchor), the anchor
//                               fastest, so the stores of a wave are 256 contiguous bytes per value;
//                       gather  behind dy_nms: out[b, r, 0:nk] for the kept rows r < counts[b] from anchor index[b, r]: thread = (image,
//                               row, keypoint), the keypoint fastest, so a wave reads and writes runs of contiguous floats.
//   dy_scale_coords   PosePredictor.construct_result's ops.scale_coords (utils/ops.py:756-788) and the Keypoints constructor's masking of
//                     invisible points (engine/results.py:1373-1375), in place on the gathered rows; a crop's offset is added last, to the
//                     keypoints and -- behind dy_scale_boxes -- to the row's box.
//   dy_crops_letterbox_u8_to_nchw_f32
//                     k windows of f frames, each letterboxed to (hn, wn) as dy_letterbox_u8_to_nchw_f32 letterboxes a contiguous copy of the
//                     window (letterbox_px.h: the one copy of the interpolation).  Memory-bound (12 bytes written per output pixel): a lane
//                     owns four consecutive x of one output row -- three float4 stores where wn % 4 == 0 and dst is 16-byte aligned --
//                     and the grid is (runs of 256 quads of a crop, crop): one 640 x 640 crop is 400 workgroups, 256 crops 102,400.
//
// fp32 in the reference's order of operations with contraction off.  expf is the device's and is not bit-equal to the CPU's: the visibility
// agrees to a few ulp (tools/make_pose_golden.py records the bound), x and y are bit-equal.
#include "letterbox_px.h"

#pragma clang fp contract(off)

namespace dy {

constexpr int kMaxNk = 256;

struct KptArgs {
  const float* level[DY_MAX_LEVELS];
  int w[DY_MAX_LEVELS], hw[DY_MAX_LEVELS], ld[DY_MAX_LEVELS], a0[DY_MAX_LEVELS + 1];  // a0: first anchor of the level
  float stride[DY_MAX_LEVELS];
  int n_levels, batch, anchors, nkpt, ndim, max_det;
  float* pred_kpt;
  const int* counts;
  const int* index;
  float* out;
};

// One keypoint of one anchor.  p: its ndim logits; (col, row): the anchor's cell, s: the level's stride.  The reference computes
// (y * 2.0 + (anchor - 0.5)) * stride with anchor = cell + 0.5 (tal.py make_anchors), every step rounded to fp32.
__device__ __forceinline__ void kpt_one(const float* p, int ndim, int col, int row, float s, float* o) {
  const float ax = ((float)col + 0.5f) - 0.5f, ay = ((float)row + 0.5f) - 0.5f;
  o[0] = (p[0] * 2.0f + ax) * s;
  o[1] = (p[1] * 2.0f + ay) * s;
  if (ndim == 3) o[2] = 1.f / (1.f + expf(-p[2]));
}

__device__ __forceinline__ const float* kpt_anchor(const KptArgs& a, int b, int an, int* col, int* row, float* s) {
  int l = 0;
  while (l + 1 < a.n_levels && an >= a.a0[l + 1]) ++l;
  const int pix = an - a.a0[l];
  *row = pix / a.w[l];
  *col = pix - *row * a.w[l];
  *s = a.stride[l];
  return a.level[l] + ((size_t)b * a.hw[l] + pix) * (size_t)a.ld[l];
}

__global__ __launch_bounds__(256) void kpt_decode_dense_kernel(const KptArgs a) {
  const long long total = (long long)a.batch * a.nkpt * a.anchors;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int an = (int)(i % a.anchors);
    const long long t = i / a.anchors;
    const int k = (int)(t % a.nkpt), b = (int)(t / a.nkpt);
    int col, row;
    float s, o[3];
    const float* p = kpt_anchor(a, b, an, &col, &row, &s) + k * a.ndim;
    kpt_one(p, a.ndim, col, row, s, o);
    float* d = a.pred_kpt + ((size_t)b * a.nkpt * a.ndim + (size_t)k * a.ndim) * a.anchors + an;
    for (int c = 0; c < a.ndim; ++c) d[(size_t)c * a.anchors] = o[c];
  }
}

__global__ __launch_bounds__(256) void kpt_decode_gather_kernel(const KptArgs a) {
  const long long total = (long long)a.batch * a.max_det * a.nkpt;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % a.nkpt);
    const long long br = i / a.nkpt;
    const int r = (int)(br % a.max_det), b = (int)(br / a.max_det);
    if (r >= a.counts[b]) continue;  // rows beyond the count: neither read nor written
    float o[3] = {0.f, 0.f, 0.f};
    const int an = a.index[br];
    if (an >= 0 && an < a.anchors) {
      int col, row;
      float s;
      const float* p = kpt_anchor(a, b, an, &col, &row, &s) + k * a.ndim;
      kpt_one(p, a.ndim, col, row, s, o);
    }
    float* d = a.out + (size_t)i * a.ndim;
    for (int c = 0; c < a.ndim; ++c) d[c] = o[c];
  }
}

// scale_coords + clip_coords, then Keypoints' `keypoints[..., :2][mask] = 0` for conf < 0.5, then the crop's offset.
__global__ __launch_bounds__(256) void scale_coords_kernel(float* __restrict__ kpts, float* __restrict__ boxes, const int* __restrict__ counts,
                                                           const float* __restrict__ params, int batch, int max_det, int nkpt, int ndim) {
  const long long total = (long long)batch * max_det * nkpt;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long br = i / nkpt;
    const int r = (int)(br % max_det), b = (int)(br / max_det);
    if (r >= counts[b]) continue;
    const float* q = params + (size_t)b * 7;
    const float gain = q[0], px = q[1], py = q[2], cw = q[3], ch = q[4], ox = q[5], oy = q[6];
    float* o = kpts + (size_t)i * ndim;
    float x = fminf(fmaxf((o[0] - px) / gain, 0.f), cw);
    float y = fminf(fmaxf((o[1] - py) / gain, 0.f), ch);
    if (ndim == 3 && o[2] < 0.5f) {
      x = 0.f, y = 0.f;
    } else {
      x = x + ox, y = y + oy;
    }
    o[0] = x, o[1] = y;
    if (boxes && i == br * nkpt && (ox != 0.f || oy != 0.f)) {  // the row's first keypoint also shifts the row's box (already scaled and clamped)
      float* bx = boxes + (size_t)br * 6;
      bx[0] = bx[0] + ox, bx[1] = bx[1] + oy, bx[2] = bx[2] + ox, bx[3] = bx[3] + oy;
    }
  }
}

// ---- crop slicer ----------------------------------------------------------------------------------------------------------------------
constexpr int kCropCols = 9;  // frame, x0, y0, cw, ch, new_w, new_h, top, left

struct CropArgs {
  const uint8_t* frames;
  const int* table;
  float* dst;
  int f, hf, wf, k, hn, wn, swap_rb;
  float pad;
};

// Whether a table row describes a window inside its frame and a resized image inside the output (host and device ask the same question).
__host__ __device__ inline bool crop_row_ok(const int* t, int f, int hf, int wf, int hn, int wn) {
  return t[0] >= 0 && t[0] < f && t[3] >= 1 && t[4] >= 1 && t[1] >= 0 && t[2] >= 0 && t[1] <= wf - t[3] && t[2] <= hf - t[4] && t[5] >= 1 && t[6] >= 1 &&
         t[7] >= 0 && t[8] >= 0 && t[6] <= hn - t[7] && t[5] <= wn - t[8];
}

template <bool VEC>
__global__ __launch_bounds__(256) void crops_letterbox_kernel(const CropArgs p) {
  const int crop = blockIdx.y;  // workgroup-uniform: the table row comes in through scalar loads
  const int* t = p.table + (size_t)crop * kCropCols;
  const int qw = (p.wn + 3) >> 2;  // quads of four x per output row
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.hn * qw) return;
  const int y = i / qw, x = (i - y * qw) * 4;
  const float padv = p.pad / 255.0f;
  float c0[4], c1[4], c2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c0[j] = c1[j] = c2[j] = padv;
  const int fr = t[0], x0 = t[1], y0 = t[2], cw = t[3], ch = t[4], new_w = t[5], new_h = t[6], top = t[7], left = t[8];
  const int ry = y - top;
  // (the host refused a bad row before the launch; a table that differs from the one it checked still reads nothing outside the frames)
  if (crop_row_ok(t, p.f, p.hf, p.wf, p.hn, p.wn) && (unsigned)ry < (unsigned)new_h && x + 3 >= left && x < left + new_w) {
    const size_t pitch = (size_t)p.wf * 3;
    const uint8_t* s = p.frames + (size_t)fr * p.hf * pitch + (size_t)y0 * pitch + (size_t)x0 * 3;
    const bool copy = new_h == ch && new_w == cw;
    const double sx = __ddiv_rn((double)cw, (double)new_w), sy = __ddiv_rn((double)ch, (double)new_h);
    LbRow row{};
    if (!copy) row = letterbox_row(ry, sy, ch);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rx = x + j - left;
      if ((unsigned)rx < (unsigned)new_w) {
        float v[3];
        letterbox_px(s, pitch, ch, cw, new_h, new_w, sx, row, ry, rx, v);
        c0[j] = v[0] / 255.0f, c1[j] = v[1] / 255.0f, c2[j] = v[2] / 255.0f;
      }
    }
  }
  const size_t plane = (size_t)p.hn * p.wn;
  float* d = p.dst + (size_t)crop * 3 * plane + (size_t)y * p.wn + x;
  const float* first = p.swap_rb ? c2 : c0;
  const float* last = p.swap_rb ? c0 : c2;
  if (VEC) {  // wn % 4 == 0 and dst 16-byte aligned: every quad is one aligned float4 per plane
    *reinterpret_cast<float4*>(d) = make_float4(first[0], first[1], first[2], first[3]);
    *reinterpret_cast<float4*>(d + plane) = make_float4(c1[0], c1[1], c1[2], c1[3]);
    *reinterpret_cast<float4*>(d + 2 * plane) = make_float4(last[0], last[1], last[2], last[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < p.wn) {
        d[j] = first[j];
        d[plane + j] = c1[j];
        d[2 * plane + j] = last[j];
      }
  }
}

static inline unsigned pose_grid_for(long long total) {
  long long g = (total + 255) / 256;
  if (g < 1) g = 1;
  if (g > 65536) g = 65536;
  return (unsigned)g;
}

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_kpt_decode(const dy_kpt_decode_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d, DY_ERR_INVALID_ARG, "dy_kpt_decode: null descriptor");
  DY_REQUIRE(d->ndim == 2 || d->ndim == 3, DY_ERR_UNSUPPORTED, "dy_kpt_decode: %d values per keypoint (built for 2 and 3)", d->ndim);
  DY_REQUIRE(d->nkpt > 0 && (long long)d->nkpt * d->ndim <= kMaxNk, d->nkpt > 0 ? DY_ERR_UNSUPPORTED : DY_ERR_INVALID_ARG,
             "dy_kpt_decode: nk = %lld keypoint values (1 .. %d)", (long long)d->nkpt * d->ndim, kMaxNk);
  DY_REQUIRE((d->pred_kpt != nullptr) != (d->out != nullptr), DY_ERR_INVALID_ARG, "dy_kpt_decode: give pred_kpt (dense form) or out (gather form)");
  DY_REQUIRE(d->batch > 0 && d->anchors > 0, DY_ERR_INVALID_ARG, "dy_kpt_decode: bad dims");
  DY_REQUIRE(d->n_levels > 0 && d->n_levels <= DY_MAX_LEVELS, DY_ERR_INVALID_ARG, "dy_kpt_decode: bad n_levels");
  const int nk = d->nkpt * d->ndim;
  KptArgs a{};
  long long A = 0;
  for (int i = 0; i < d->n_levels; ++i) {
    DY_REQUIRE(d->level[i] && d->h[i] > 0 && d->w[i] > 0 && d->ld[i] >= nk && d->stride[i] > 0.f, DY_ERR_INVALID_ARG, "dy_kpt_decode: bad level %d", i);
    DY_REQUIRE((long long)d->h[i] * d->w[i] <= 0x7fffffffll, DY_ERR_INVALID_ARG, "dy_kpt_decode: level %d too large", i);
    a.level[i] = d->level[i], a.w[i] = d->w[i], a.hw[i] = d->h[i] * d->w[i], a.ld[i] = d->ld[i], a.stride[i] = d->stride[i];
    a.a0[i] = (int)A;
    A += (long long)d->h[i] * d->w[i];
    DY_REQUIRE(A <= 0x7fffffffll, DY_ERR_INVALID_ARG, "dy_kpt_decode: too many anchors");
  }
  a.a0[d->n_levels] = (int)A;
  DY_REQUIRE(A == d->anchors, DY_ERR_INVALID_ARG, "dy_kpt_decode: the levels hold %lld anchors, anchors = %d", A, d->anchors);
  a.n_levels = d->n_levels, a.batch = d->batch, a.anchors = d->anchors, a.nkpt = d->nkpt, a.ndim = d->ndim;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->pred_kpt) {
    a.pred_kpt = d->pred_kpt;
    hipLaunchKernelGGL(kpt_decode_dense_kernel, dim3(pose_grid_for((long long)d->batch * d->nkpt * d->anchors)), dim3(256), 0, st, a);
    return check_launch("kpt_decode_dense_kernel");
  }
  DY_REQUIRE(d->counts && d->index && d->max_det > 0, DY_ERR_INVALID_ARG, "dy_kpt_decode: the gather form needs counts, index and max_det > 0");
  a.counts = d->counts, a.index = d->index, a.out = d->out, a.max_det = d->max_det;
  hipLaunchKernelGGL(kpt_decode_gather_kernel, dim3(pose_grid_for((long long)d->batch * d->max_det * d->nkpt)), dim3(256), 0, st, a);
  return check_launch("kpt_decode_gather_kernel");
}

extern "C" int32_t dy_scale_coords(float* kpts, float* boxes, const int32_t* counts, const float* params, int32_t batch, int32_t max_det, int32_t nkpt,
                                   int32_t ndim, dy_stream_t stream) {
  DY_REQUIRE(kpts && counts && params, DY_ERR_INVALID_ARG, "dy_scale_coords: null pointer");
  DY_REQUIRE(batch > 0 && max_det > 0 && nkpt > 0, DY_ERR_INVALID_ARG, "dy_scale_coords: bad dims");
  DY_REQUIRE(ndim == 2 || ndim == 3, DY_ERR_UNSUPPORTED, "dy_scale_coords: %d values per keypoint (built for 2 and 3)", ndim);
  DY_REQUIRE((long long)nkpt * ndim <= kMaxNk, DY_ERR_UNSUPPORTED, "dy_scale_coords: more than %d keypoint values", kMaxNk);
  hipLaunchKernelGGL(scale_coords_kernel, dim3(pose_grid_for((long long)batch * max_det * nkpt)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), kpts,
                     boxes, counts, params, batch, max_det, nkpt, ndim);
  return check_launch("scale_coords_kernel");
}

extern "C" int32_t dy_crops_letterbox_u8_to_nchw_f32(const uint8_t* frames, const int32_t* table, const int32_t* table_host, float* dst, int32_t f, int32_t hf,
                                                     int32_t wf, int32_t k, int32_t hn, int32_t wn, int32_t swap_rb, float pad_value, dy_stream_t stream) {
  DY_REQUIRE(frames && table && table_host && dst, DY_ERR_INVALID_ARG, "dy_crops_letterbox_u8_to_nchw_f32: null pointer");
  DY_REQUIRE(f > 0 && hf > 0 && wf > 0 && k > 0 && hn > 0 && wn > 0, DY_ERR_INVALID_ARG, "dy_crops_letterbox_u8_to_nchw_f32: bad dims");
  DY_REQUIRE(k <= 65535, DY_ERR_INVALID_ARG, "dy_crops_letterbox_u8_to_nchw_f32: %d crops in one launch (at most 65535)", k);
  DY_REQUIRE((long long)hn * ((wn + 3) / 4) <= 0x7fffffffll / 2 && (long long)hf * wf * 3 <= 0x7fffffffll, DY_ERR_INVALID_ARG,
             "dy_crops_letterbox_u8_to_nchw_f32: output or frame too large");
  for (int j = 0; j < k; ++j) {
    const int32_t* t = table_host + (size_t)j * kCropCols;
    DY_REQUIRE(crop_row_ok(t, f, hf, wf, hn, wn), DY_ERR_INVALID_ARG,
               "dy_crops_letterbox_u8_to_nchw_f32: crop %d (frame %d, %dx%d at %d,%d -> %dx%d at %d,%d) leaves its %dx%d frame or the %dx%d output", j, t[0], t[3],
               t[4], t[1], t[2], t[5], t[6], t[8], t[7], wf, hf, wn, hn);
  }
  CropArgs a{};
  a.frames = frames, a.table = table, a.dst = dst, a.f = f, a.hf = hf, a.wf = wf, a.k = k, a.hn = hn, a.wn = wn, a.swap_rb = swap_rb ? 1 : 0, a.pad = pad_value;
  const dim3 grid((unsigned)(((long long)hn * ((wn + 3) / 4) + 255) / 256), (unsigned)k);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (wn % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0)
    hipLaunchKernelGGL(crops_letterbox_kernel<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(crops_letterbox_kernel<false>, grid, dim3(256), 0, st, a);
  return check_launch("dy_crops_letterbox_u8_to_nchw_f32");
}
