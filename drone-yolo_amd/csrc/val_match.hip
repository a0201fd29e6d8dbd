// Validation matching on the padded dy_nms output: BaseValidator.match_predictions (engine/validator.py:224-264, the non-scipy
// branch) with the box_iou it is fed (utils/metrics.py:52-71), for a whole batch in one launch.
//
// The reference's per-threshold nonzero / argsort / unique / unique collapses to two facts per detection d (rows are in descending
// confidence, so "d' < d" is "ranked higher"):
//     best(d) = argmax_l m(l, d),  biou(d) = max_l m(l, d),   m(l, d) = iou(l, d) if tcls[l] == cls[d] else 0,  l over the image's labels
//     correct(d, t)  <=>  biou(d) >= t  and no d' < d has best(d') == best(d) and biou(d') >= t
// (sorted by IoU, the first unique keeps every detection's best label among those >= t, which is best(d) whenever biou(d) >= t; the
// second unique keeps a label's lowest-indexed detection).  Exact ties for best(d) go to the label that comes first in tbox: the
// reference resolves them through an unstable sort, so its order is not defined.
//
//   val_match_kernel   one workgroup (512 threads) per image.  The image's detections (clipped box, class) and their best / biou sit
//                      in LDS.  The batch's labels are streamed in steps of VM_STEP: every thread looks at the image index of its
//                      labels and appends the ones of this image (box, area, class, position) to an LDS stage, then every thread
//                      runs its detections (tid, tid + 512, ...) over the stage.  Labels per image are unbounded: nothing is sized
//                      by them.  The scan over d' < d reads best / biou of the max_det staged detections only.
//
// The IoU follows box_iou operation by operation in fp32 with contraction off and the correctly rounded division, so biou is
// bit-equal to the host's value and the ">= t" verdicts are the host's:
//     inter = max(min(x2) - max(x1), 0) * max(min(y2) - max(y1), 0);  iou = inter / (((w1 * h1) + (w2 * h2)) - inter + 1e-7f)
// A pair of another class or without overlap is m = 0 exactly (0 / positive), so the division runs for overlapping same-class pairs only.
#include "common_hip.h"
#include "val_scan.h"

#pragma clang fp contract(off)

namespace dy {

constexpr int VM_THREADS = 512;  // one detection per thread at the validator's max_det 300; eight waves hide the LDS latency of the label loop
constexpr int VM_STEP = 512;      // labels looked at per step = capacity of the LDS stage
constexpr int VM_MAX_IOUV = 16;
constexpr int VM_MAX_DET = 4096;  // dy_nms's bound; 32 B of LDS per detection

struct ValMatchArgs {
  const float* rows;
  const int* counts;
  const float* tbox;
  const float* tcls;
  const int* timg;
  int batch, max_det, n_labels, n_iouv;
  float clip_w, clip_h;
  int single_cls;
  float iouv[VM_MAX_IOUV];
  uint8_t* tp;
  float* best_iou;
  int* best_label;
};

static inline size_t val_match_lds_bytes(int max_det) { return (size_t)VM_STEP * 32 + (size_t)max_det * 32 + 16 + VM_MAX_IOUV * 4; }

__global__ __launch_bounds__(VM_THREADS) void val_match_kernel(const ValMatchArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  float4* lbox = reinterpret_cast<float4*>(dyn_smem);            // [VM_STEP] the stage: this image's labels of the current step
  float4* dbox = lbox + VM_STEP;                                 // [max_det] clipped detections
  float4* lmeta = dbox + p.max_det;                              // [VM_STEP] area, class, position in tbox (int bits), unused
  float* dcls = reinterpret_cast<float*>(lmeta + VM_STEP);       // [max_det]
  float* biou = dcls + p.max_det;                                // [max_det]
  int* best = reinterpret_cast<int*>(biou + p.max_det);          // [max_det]
  float* prev = reinterpret_cast<float*>(best + p.max_det);      // [max_det] max biou(d') over d' < d with best(d') == best(d)
  int* n_staged = reinterpret_cast<int*>(prev + p.max_det);      // labels staged so far, all steps together (never reset)
  float* thr = reinterpret_cast<float*>(n_staged + 4);           // [VM_MAX_IOUV] the thresholds (indexed per element below)
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  int cnt = p.counts[b];
  cnt = cnt < 0 ? 0 : (cnt > p.max_det ? p.max_det : cnt);

  const float* rb = p.rows + (size_t)b * p.max_det * 6;
  for (int d = tid; d < cnt; d += VM_THREADS) {
    const float* r = rb + (size_t)d * 6;
    // the clip of _prepare_pred (ops.clip_boxes): min(max(x, 0), w)
    dbox[d] = make_float4(fminf(fmaxf(r[0], 0.f), p.clip_w), fminf(fmaxf(r[1], 0.f), p.clip_h), fminf(fmaxf(r[2], 0.f), p.clip_w),
                          fminf(fmaxf(r[3], 0.f), p.clip_h));
    dcls[d] = p.single_cls ? 0.f : r[5];
    biou[d] = -1.f;  // below every m: the first label of the image always takes an empty slot
    best[d] = -1;
  }

  if (tid == 0) *n_staged = 0;
#pragma unroll
  for (int i = 0; i < VM_MAX_IOUV; ++i)
    if (tid == i) thr[i] = p.iouv[i];
  __syncthreads();
  int seen = 0;  // the counter after the previous step
  for (int l0 = 0; l0 < p.n_labels && cnt > 0; l0 += VM_STEP) {  // (cnt is the same on every thread: the barriers are uniform)
    for (int l = l0 + tid; l < l0 + VM_STEP && l < p.n_labels; l += VM_THREADS) {
      if (p.timg[l] != b) continue;
      const int at = atomicAdd(n_staged, 1) - seen;  // the stage is unordered; the tie rule below restores tbox order
      const float4 t = reinterpret_cast<const float4*>(p.tbox)[l];
      lbox[at] = t;
      lmeta[at] = make_float4((t.z - t.x) * (t.w - t.y), p.tcls[l], __int_as_float(l), 0.f);
    }
    __syncthreads();
    const int ns = *n_staged - seen;  // at most VM_STEP: one entry per label looked at
    seen += ns;
    for (int d = tid; d < cnt && ns > 0; d += VM_THREADS) {
      const float4 q = dbox[d];
      const float qc = dcls[d];
      const float qar = (q.z - q.x) * (q.w - q.y);
      float bi = biou[d];
      int bl = best[d];
#pragma unroll 4
      for (int k = 0; k < ns; ++k) {  // (every lane reads the same stage entry: LDS broadcasts; unrolled so that the reads of four entries are in flight)
        const float4 t = lbox[k];
        const float4 mt = lmeta[k];
        const float w = fmaxf(fminf(t.z, q.z) - fmaxf(t.x, q.x), 0.f);
        const float h = fmaxf(fminf(t.w, q.w) - fmaxf(t.y, q.y), 0.f);
        const float inter = w * h;
        float m = 0.f;
        if (inter > 0.f && mt.y == qc) {
          const float sum = mt.x + qar;
          const float uni = sum - inter;
          m = __fdiv_rn(inter, uni + 1e-7f);
        }
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

  // the rank scan over d' < d and the stores (val_scan.h, shared with dy_val_mask_match)
  val_rank_scan(best, biou, prev, thr, cnt, p.max_det, p.n_iouv, p.tp + (size_t)b * p.max_det * p.n_iouv,
                p.best_iou ? p.best_iou + (size_t)b * p.max_det : nullptr, p.best_label ? p.best_label + (size_t)b * p.max_det : nullptr, 0, tid, VM_THREADS);
}

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_val_match(const dy_val_match_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->rows && d->counts && d->tp, DY_ERR_INVALID_ARG, "dy_val_match: null pointer (rows / counts / tp)");
  DY_REQUIRE(d->batch > 0 && d->max_det > 0 && d->max_det <= VM_MAX_DET, DY_ERR_INVALID_ARG,
             "dy_val_match: bad dims (batch %d, max_det %d; max_det must be in [1,%d])", d->batch, d->max_det, VM_MAX_DET);
  DY_REQUIRE(d->n_iouv >= 1 && d->n_iouv <= VM_MAX_IOUV && d->iouv, DY_ERR_INVALID_ARG, "dy_val_match: n_iouv %d must be in [1,%d] with iouv set",
             d->n_iouv, VM_MAX_IOUV);
  DY_REQUIRE(d->n_labels >= 0, DY_ERR_INVALID_ARG, "dy_val_match: n_labels %d < 0", d->n_labels);
  DY_REQUIRE(d->n_labels == 0 || (d->tbox && d->tcls && d->timg), DY_ERR_INVALID_ARG, "dy_val_match: null label pointer with n_labels %d", d->n_labels);
  DY_REQUIRE(d->n_labels == 0 || aligned16(d->tbox), DY_ERR_INVALID_ARG, "dy_val_match: tbox not 16-byte aligned");
  ValMatchArgs a{};
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
  static const hipError_t attr_once = hipFuncSetAttribute((const void*)val_match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)attr_once;
  hipLaunchKernelGGL(val_match_kernel, dim3((unsigned)d->batch), dim3(VM_THREADS), val_match_lds_bytes(d->max_det),
                     reinterpret_cast<hipStream_t>(stream), a);
  return check_launch("val_match_kernel");
}
