// Validation matching of oriented boxes on the padded dy_nms_rotated / dy_nms_rotated_ml output: OBBValidator._process_batch
// (models/yolo/obb/val.py: match_predictions on iou = batch_probiou(gt, det)) with the clip of _prepare_pred, for a whole batch in one
// launch.  The match rule is val_match.hip's:
//     best(d) = argmax_l m(l, d),  biou(d) = max_l m(l, d),   m(l, d) = probiou(l, d) if tcls[l] == cls[d] else 0,  l over the image's labels
//     correct(d, t)  <=>  biou(d) >= t  and no d' < d has best(d') == best(d) and biou(d') >= t          (val_scan.h)
// Exact ties for best(d) go to the label that comes first in tbox; a NaN m (a degenerate pair whose determinant rounds below zero) compares
// false both ways and never becomes the best.
//
//   val_match_rotated_kernel   one workgroup (512 threads) per image.  The image's detections are clipped as scale_boxes(xywh=True) at gain
//                      1 / pad 0 leaves them (clip_boxes: columns 0 and 2 to [0, clip_w], 1 and 3 to [0, clip_h] -- the width and height
//                      too; theta untouched, not regularized) and their five ProbIoU floats (x, y and the covariance terms a, b, c:
//                      probiou.h) and class are computed once into LDS.  The batch's labels are streamed in steps of VR_STEP: every thread
//                      looks at the image index of its labels and appends the ones of this image (five floats, class, position) to an LDS
//                      stage, so a label's covariance terms are computed once per image, not once per pair; then every thread runs its
//                      detections (tid, tid + 512, ...) over the stage with broadcast reads.  Nothing is sized by the labels of one image.
//
// probiou.h is the NMS's expression (fp32, the reference's order of operations, contraction off).  sinf / cosf / logf / expf are the
// device's and not bit-equal to the CPU's: tp equals the host's for inputs the reference decides with a margin (tools/make_obbval_golden.py).
#include "common_hip.h"
#include "probiou.h"
#include "val_scan.h"

#pragma clang fp contract(off)

namespace dy {

constexpr int VR_THREADS = 512;  // one detection per thread at the validator's max_det 300
constexpr int VR_STEP = 256;     // labels looked at per step = capacity of the LDS stage (8 KB: with 36 B per detection, max_det 4096 stays under the 160 KB of a CU)
constexpr int VR_MAX_IOUV = 16;
constexpr int VR_MAX_DET = 4096;  // dy_nms_rotated's bound; 36 B of LDS per detection

struct ValMatchRArgs {
  const float* rows;
  const int* counts;
  const float* tbox;
  const float* tcls;
  const int* timg;
  int batch, max_det, n_labels, n_iouv;
  float clip_w, clip_h;
  int single_cls;
  float iouv[VR_MAX_IOUV];
  uint8_t* tp;
  float* best_iou;
  int* best_label;
};

static inline size_t val_match_rotated_lds_bytes(int max_det) { return (size_t)VR_STEP * 32 + (size_t)max_det * 36 + 16 + VR_MAX_IOUV * 4; }

__global__ __launch_bounds__(VR_THREADS) void val_match_rotated_kernel(const ValMatchRArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  float4* lrow = reinterpret_cast<float4*>(dyn_smem);        // [VR_STEP] the stage: x, y, a, b of this image's labels of the current step
  float4* lmeta = lrow + VR_STEP;                            // [VR_STEP] c, class, position in tbox (int bits), unused
  float4* drow = lmeta + VR_STEP;                            // [max_det] x, y, a, b of the clipped detections
  float* dc = reinterpret_cast<float*>(drow + p.max_det);    // [max_det] their c
  float* dcls = dc + p.max_det;                              // [max_det]
  float* biou = dcls + p.max_det;                            // [max_det]
  int* best = reinterpret_cast<int*>(biou + p.max_det);      // [max_det]
  float* prev = reinterpret_cast<float*>(best + p.max_det);  // [max_det] val_rank_scan's scratch
  int* n_staged = reinterpret_cast<int*>(prev + p.max_det);  // labels staged so far, all steps together (never reset)
  float* thr = reinterpret_cast<float*>(n_staged + 4);       // [VR_MAX_IOUV]
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  int cnt = p.counts[b];
  cnt = cnt < 0 ? 0 : (cnt > p.max_det ? p.max_det : cnt);

  const float* rb = p.rows + (size_t)b * p.max_det * 7;
  for (int d = tid; d < cnt; d += VR_THREADS) {
    const float* r = rb + (size_t)d * 7;
    // the clip of _prepare_pred (scale_boxes(xywh=True) at gain 1, pad 0 -> clip_boxes): min(max(v, 0), limit) on x, y, w AND h
    const RRow q = rnms_row(fminf(fmaxf(r[0], 0.f), p.clip_w), fminf(fmaxf(r[1], 0.f), p.clip_h), fminf(fmaxf(r[2], 0.f), p.clip_w),
                            fminf(fmaxf(r[3], 0.f), p.clip_h), r[4]);
    drow[d] = make_float4(q.x, q.y, q.a, q.b);
    dc[d] = q.c;
    dcls[d] = p.single_cls ? 0.f : r[6];
    biou[d] = -1.f;  // below every m: the first label of the image always takes an empty slot (a NaN m does not)
    best[d] = -1;
  }

  if (tid == 0) *n_staged = 0;
#pragma unroll
  for (int i = 0; i < VR_MAX_IOUV; ++i)
    if (tid == i) thr[i] = p.iouv[i];
  __syncthreads();
  int seen = 0;  // the counter after the previous step
  for (int l0 = 0; l0 < p.n_labels && cnt > 0; l0 += VR_STEP) {  // (cnt is the same on every thread: the barriers are uniform)
    for (int l = l0 + tid; l < l0 + VR_STEP && l < p.n_labels; l += VR_THREADS) {
      if (p.timg[l] != b) continue;
      const int at = atomicAdd(n_staged, 1) - seen;  // the stage is unordered; the tie rule below restores tbox order
      const float4 t0 = reinterpret_cast<const float4*>(p.tbox)[2 * (size_t)l];  // x, y, w, h
      const float th = p.tbox[8 * (size_t)l + 4];
      const RRow r = rnms_row(t0.x, t0.y, t0.z, t0.w, th);
      lrow[at] = make_float4(r.x, r.y, r.a, r.b);
      lmeta[at] = make_float4(r.c, p.tcls[l], __int_as_float(l), 0.f);
    }
    __syncthreads();
    const int ns = *n_staged - seen;  // at most VR_STEP: one entry per label looked at
    seen += ns;
    for (int d = tid; d < cnt && ns > 0; d += VR_THREADS) {
      const float4 q4 = drow[d];
      const RRow q{q4.x, q4.y, q4.z, q4.w, dc[d]};
      const float qc = dcls[d];
      float bi = biou[d];
      int bl = best[d];
      for (int k = 0; k < ns; ++k) {  // (every lane reads the same stage entry: LDS broadcasts)
        const float4 t = lrow[k];
        const float4 mt = lmeta[k];
        float m = 0.f;
        if (mt.y == qc) m = rnms_probiou(RRow{t.x, t.y, t.z, t.w, mt.x}, q);  // batch_probiou(gt, det)
        const int l = __float_as_int(mt.z);
        if (m > bi || (m == bi && l < bl)) {
          bi = m;
          bl = l;
        }
      }
      biou[d] = bi;
      best[d] = bl;
    }
    __syncthreads();  // the stage is rewritten and the counter moves on in the next step
  }

  val_rank_scan(best, biou, prev, thr, cnt, p.max_det, p.n_iouv, p.tp + (size_t)b * p.max_det * p.n_iouv,
                p.best_iou ? p.best_iou + (size_t)b * p.max_det : nullptr, p.best_label ? p.best_label + (size_t)b * p.max_det : nullptr, 0, tid, VR_THREADS);
}

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_val_match_rotated(const dy_val_match_rotated_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->rows && d->counts && d->tp, DY_ERR_INVALID_ARG, "dy_val_match_rotated: null pointer (rows / counts / tp)");
  DY_REQUIRE(d->batch > 0 && d->max_det > 0 && d->max_det <= VR_MAX_DET, DY_ERR_INVALID_ARG,
             "dy_val_match_rotated: bad dims (batch %d, max_det %d; max_det must be in [1,%d])", d->batch, d->max_det, VR_MAX_DET);
  DY_REQUIRE(d->n_iouv >= 1 && d->n_iouv <= VR_MAX_IOUV && d->iouv, DY_ERR_INVALID_ARG,
             "dy_val_match_rotated: n_iouv %d must be in [1,%d] with iouv set", d->n_iouv, VR_MAX_IOUV);
  DY_REQUIRE(d->n_labels >= 0, DY_ERR_INVALID_ARG, "dy_val_match_rotated: n_labels %d < 0", d->n_labels);
  DY_REQUIRE(d->n_labels == 0 || (d->tbox && d->tcls && d->timg), DY_ERR_INVALID_ARG, "dy_val_match_rotated: null label pointer with n_labels %d",
             d->n_labels);
  DY_REQUIRE(d->n_labels == 0 || aligned16(d->tbox), DY_ERR_INVALID_ARG, "dy_val_match_rotated: tbox not 16-byte aligned");
  ValMatchRArgs a{};
  a.rows = d->rows;
  a.counts = d->counts;
  a.tbox = d->tbox;
  a.tcls = d->tcls;
  a.timg = d->timg;
  a.batch = d->batch;
  a.max_det = d->max_det;
  a.n_labels = d->n_labels;
  a.n_iouv = d->n_iouv;
  a.clip_w = d->clip_w;
  a.clip_h = d->clip_h;
  a.single_cls = d->single_cls;
  for (int i = 0; i < d->n_iouv; ++i) a.iouv[i] = d->iouv[i];
  a.tp = d->tp;
  a.best_iou = d->best_iou;
  a.best_label = d->best_label;
  static const hipError_t attr_once =
      hipFuncSetAttribute((const void*)val_match_rotated_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)attr_once;
  hipLaunchKernelGGL(val_match_rotated_kernel, dim3((unsigned)d->batch), dim3(VR_THREADS), val_match_rotated_lds_bytes(d->max_det),
                     reinterpret_cast<hipStream_t>(stream), a);
  return check_launch("val_match_rotated_kernel");
}
