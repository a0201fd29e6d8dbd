// Validation matching on the padded NMS output, for a whole batch in one launch: BaseValidator.match_predictions (engine/validator.py:224-264,
// the non-scipy branch) on the pair score its validator feeds it.  One kernel template, two policies:
//     dy_val_match          VmBox      box_iou (utils/metrics.py:52-71) on the dy_nms rows, clipped as _prepare_pred clips them
//     dy_val_match_rotated  VmRotated  batch_probiou(gt, det) (OBBValidator._process_batch, models/yolo/obb/val.py) on the dy_nms_rotated /
//                                      dy_nms_rotated_ml rows, clipped as scale_boxes(xywh=True) at gain 1 / pad 0 leaves them
//
// The reference's per-threshold nonzero / argsort / unique / unique collapses to two facts per detection d (rows are in descending
// confidence, so "d' < d" is "ranked higher"):
//     best(d) = argmax_l m(l, d),  biou(d) = max_l m(l, d),   m(l, d) = score(l, d) if tcls[l] == cls[d] else 0,  l over the image's labels
//     correct(d, t)  <=>  biou(d) >= t  and no d' < d has best(d') == best(d) and biou(d') >= t          (val_scan.h)
// (sorted by IoU, the first unique keeps every detection's best label among those >= t, which is best(d) whenever biou(d) >= t; the
// second unique keeps a label's lowest-indexed detection).  Exact ties for best(d) go to the label that comes first in tbox: the
// reference resolves them through an unstable sort, so its order is not defined.  A NaN m (a degenerate rotated pair whose determinant
// rounds below zero) compares false both ways and never becomes the best.
//
//   val_match_kernel_t   one workgroup (512 threads) per image.  The image's detections are clipped and converted once (Policy::stage_det)
//                      and sit in LDS with their class and their best / biou.  The batch's labels are streamed in steps of Policy::STEP:
//                      every thread looks at the image index of its labels and appends the ones of this image (Policy::stage_label: the
//                      converted label, class, position) to an LDS stage, so a label is converted once per image, not once per pair; then
//                      every thread runs its detections (tid, tid + 512, ...) over the stage with broadcast reads.  Labels per image are
//                      unbounded: nothing is sized by them.  The scan over d' < d reads best / biou of the max_det staged detections only.
//
// VmBox follows box_iou operation by operation in fp32 with contraction off and the correctly rounded division, so biou is bit-equal to
// the host's value and the ">= t" verdicts are the host's:
//     inter = max(min(x2) - max(x1), 0) * max(min(y2) - max(y1), 0);  iou = inter / (((w1 * h1) + (w2 * h2)) - inter + 1e-7f)
// A pair of another class or without overlap is m = 0 exactly (0 / positive), so the division runs for overlapping same-class pairs only.
// VmRotated is probiou.h, the NMS's expression (fp32, the reference's order of operations, contraction off).  sinf / cosf / logf / expf are
// the device's and not bit-equal to the CPU's: tp equals the host's for inputs the reference decides with a margin (tools/make_obbval_golden.py).
#include "common_hip.h"
#include "probiou.h"
#include "val_scan.h"

#pragma clang fp contract(off)

namespace dy {

constexpr int VM_THREADS = 512;  // one detection per thread at the validator's max_det 300; eight waves hide the LDS latency of the label loop
constexpr int VM_MAX_IOUV = 16;
constexpr int VM_MAX_DET = 4096;  // dy_nms's and dy_nms_rotated's bound

struct VmItem {  // a staged label or detection: what Policy::score reads
  float4 v;
  float e;
};

struct VmBox {
  static constexpr int ROW = 6, CLS = 5;  // x1, y1, x2, y2, conf, cls
  static constexpr int STEP = 512;        // labels looked at per step = capacity of the LDS stage
  static constexpr int DET_BYTES = 16;    // LDS per detection beyond dcls / biou / best / prev: the clipped box (its area is recomputed)
  static constexpr int UNROLL = 4;        // so that the stage reads of four entries are in flight
  static __device__ __forceinline__ VmItem item(const float4& t) { return VmItem{t, (t.z - t.x) * (t.w - t.y)}; }
  // the clip of _prepare_pred (ops.clip_boxes): min(max(x, 0), w)
  static __device__ __forceinline__ VmItem stage_det(const float* r, float cw, float ch) {
    return item(make_float4(fminf(fmaxf(r[0], 0.f), cw), fminf(fmaxf(r[1], 0.f), ch), fminf(fmaxf(r[2], 0.f), cw), fminf(fmaxf(r[3], 0.f), ch)));
  }
  static __device__ __forceinline__ VmItem stage_label(const float* tbox, int l) { return item(reinterpret_cast<const float4*>(tbox)[l]); }
  static __device__ __forceinline__ VmItem load_det(const float4* dv, const float*, int d) { return item(dv[d]); }
  static __device__ __forceinline__ float score(const VmItem& t, const VmItem& q, float tcls, float qcls) {
    const float w = fmaxf(fminf(t.v.z, q.v.z) - fmaxf(t.v.x, q.v.x), 0.f);
    const float h = fmaxf(fminf(t.v.w, q.v.w) - fmaxf(t.v.y, q.v.y), 0.f);
    const float inter = w * h;
    float m = 0.f;
    if (inter > 0.f && tcls == qcls) {  // (the classes are compared here, behind the overlap: the label's class is the later LDS read)
      const float sum = t.e + q.e;
      const float uni = sum - inter;
      m = __fdiv_rn(inter, uni + 1e-7f);
    }
    return m;
  }
};

struct VmRotated {
  static constexpr int ROW = 7, CLS = 6;  // x, y, w, h, theta, conf, cls
  static constexpr int STEP = 256;        // an 8 KB stage: with 36 B per detection, max_det 4096 stays under the 160 KB of a CU
  static constexpr int DET_BYTES = 20;    // the five ProbIoU floats of probiou.h: x, y, a, b and c
  static constexpr int UNROLL = 1;
  static __device__ __forceinline__ VmItem item(const RRow& r) { return VmItem{make_float4(r.x, r.y, r.a, r.b), r.c}; }
  static __device__ __forceinline__ RRow row(const VmItem& i) { return RRow{i.v.x, i.v.y, i.v.z, i.v.w, i.e}; }
  // the clip of _prepare_pred (scale_boxes(xywh=True) at gain 1, pad 0 -> clip_boxes): min(max(v, 0), limit) on x, y, w AND h; theta is
  // untouched and not regularized
  static __device__ __forceinline__ VmItem stage_det(const float* r, float cw, float ch) {
    return item(rnms_row(fminf(fmaxf(r[0], 0.f), cw), fminf(fmaxf(r[1], 0.f), ch), fminf(fmaxf(r[2], 0.f), cw), fminf(fmaxf(r[3], 0.f), ch), r[4]));
  }
  static __device__ __forceinline__ VmItem stage_label(const float* tbox, int l) {
    const float4 t0 = reinterpret_cast<const float4*>(tbox)[2 * (size_t)l];  // x, y, w, h
    return item(rnms_row(t0.x, t0.y, t0.z, t0.w, tbox[8 * (size_t)l + 4]));
  }
  static __device__ __forceinline__ VmItem load_det(const float4* dv, const float* de, int d) { return VmItem{dv[d], de[d]}; }
  static __device__ __forceinline__ float score(const VmItem& t, const VmItem& q, float tcls, float qcls) {
    return tcls == qcls ? rnms_probiou(row(t), row(q)) : 0.f;  // batch_probiou(gt, det)
  }
};

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

// The dynamic LDS of one workgroup, as byte offsets: the kernel's pointers and the host's request both come from here.
struct VmLayout {
  unsigned lv;        // float4 [STEP]    the stage: VmItem.v of this image's labels of the current step
  unsigned dv;        // float4 [max_det] VmItem.v of the staged detections
  unsigned lmeta;     // float4 [STEP]    the stage: VmItem.e, class, position in tbox (int bits), unused
  unsigned de;        // float  [max_det] VmItem.e of the detections (DET_BYTES 20 only)
  unsigned dcls;      // float  [max_det]
  unsigned biou;      // float  [max_det]
  unsigned best;      // int    [max_det]
  unsigned prev;      // float  [max_det] val_rank_scan's scratch
  unsigned n_staged;  // int, padded to 16 B: labels staged so far, all steps together (never reset)
  unsigned thr;       // float  [VM_MAX_IOUV] the thresholds
  unsigned bytes;
};

template <class P>
__host__ __device__ inline VmLayout vm_layout(int max_det) {
  const unsigned md = (unsigned)max_det;
  VmLayout o;
  o.lv = 0;
  o.dv = o.lv + P::STEP * 16;
  o.lmeta = o.dv + md * 16;
  o.de = o.lmeta + P::STEP * 16;
  o.dcls = o.de + md * (P::DET_BYTES - 16);
  o.biou = o.dcls + md * 4;
  o.best = o.biou + md * 4;
  o.prev = o.best + md * 4;
  o.n_staged = o.prev + md * 4;
  o.thr = o.n_staged + 16;
  o.bytes = o.thr + VM_MAX_IOUV * 4;
  return o;
}

template <class P>
__global__ __launch_bounds__(VM_THREADS) void val_match_kernel_t(const ValMatchArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  const VmLayout at = vm_layout<P>(p.max_det);
  float4* lv = reinterpret_cast<float4*>(dyn_smem + at.lv);
  float4* dv = reinterpret_cast<float4*>(dyn_smem + at.dv);
  float4* lmeta = reinterpret_cast<float4*>(dyn_smem + at.lmeta);
  float* de = reinterpret_cast<float*>(dyn_smem + at.de);
  float* dcls = reinterpret_cast<float*>(dyn_smem + at.dcls);
  float* biou = reinterpret_cast<float*>(dyn_smem + at.biou);
  int* best = reinterpret_cast<int*>(dyn_smem + at.best);
  float* prev = reinterpret_cast<float*>(dyn_smem + at.prev);
  int* n_staged = reinterpret_cast<int*>(dyn_smem + at.n_staged);
  float* thr = reinterpret_cast<float*>(dyn_smem + at.thr);
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  int cnt = p.counts[b];
  cnt = cnt < 0 ? 0 : (cnt > p.max_det ? p.max_det : cnt);

  const float* rb = p.rows + (size_t)b * p.max_det * P::ROW;
  for (int d = tid; d < cnt; d += VM_THREADS) {
    const float* r = rb + (size_t)d * P::ROW;
    const VmItem q = P::stage_det(r, p.clip_w, p.clip_h);
    dv[d] = q.v;
    if (P::DET_BYTES > 16) de[d] = q.e;
    dcls[d] = p.single_cls ? 0.f : r[P::CLS];
    biou[d] = -1.f;  // below every m: the first label of the image always takes an empty slot (a NaN m does not)
    best[d] = -1;
  }

  if (tid == 0) *n_staged = 0;
#pragma unroll
  for (int i = 0; i < VM_MAX_IOUV; ++i)
    if (tid == i) thr[i] = p.iouv[i];
  __syncthreads();
  int seen = 0;  // the counter after the previous step
  for (int l0 = 0; l0 < p.n_labels && cnt > 0; l0 += P::STEP) {  // (cnt is the same on every thread: the barriers are uniform)
    for (int l = l0 + tid; l < l0 + P::STEP && l < p.n_labels; l += VM_THREADS) {
      if (p.timg[l] != b) continue;
      const int slot = atomicAdd(n_staged, 1) - seen;  // the stage is unordered; the tie rule below restores tbox order
      const VmItem t = P::stage_label(p.tbox, l);
      lv[slot] = t.v;
      lmeta[slot] = make_float4(t.e, p.tcls[l], __int_as_float(l), 0.f);
    }
    __syncthreads();
    const int ns = *n_staged - seen;  // at most STEP: one entry per label looked at
    seen += ns;
    for (int d = tid; d < cnt && ns > 0; d += VM_THREADS) {
      const VmItem q = P::load_det(dv, de, d);
      const float qc = dcls[d];
      float bi = biou[d];
      int bl = best[d];
#pragma unroll P::UNROLL
      for (int k = 0; k < ns; ++k) {  // (every lane reads the same stage entry: LDS broadcasts)
        const float4 tv = lv[k];
        const float4 mt = lmeta[k];
        const float m = P::score(VmItem{tv, mt.x}, q, mt.y, qc);  // 0 for a pair of different classes
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

// `who`: the entry point, the prefix of every refusal; `kernel_name`: what check_launch reports.
template <class P>
static int32_t launch_val_match(const dy_val_match_desc* d, dy_stream_t stream, const char* who, const char* kernel_name) {
  DY_REQUIRE(d && d->rows && d->counts && d->tp, DY_ERR_INVALID_ARG, "%s: null pointer (rows / counts / tp)", who);
  DY_REQUIRE(d->batch > 0 && d->max_det > 0 && d->max_det <= VM_MAX_DET, DY_ERR_INVALID_ARG,
             "%s: bad dims (batch %d, max_det %d; max_det must be in [1,%d])", who, d->batch, d->max_det, VM_MAX_DET);
  DY_REQUIRE(d->n_iouv >= 1 && d->n_iouv <= VM_MAX_IOUV && d->iouv, DY_ERR_INVALID_ARG, "%s: n_iouv %d must be in [1,%d] with iouv set", who,
             d->n_iouv, VM_MAX_IOUV);
  DY_REQUIRE(d->n_labels >= 0, DY_ERR_INVALID_ARG, "%s: n_labels %d < 0", who, d->n_labels);
  DY_REQUIRE(d->n_labels == 0 || (d->tbox && d->tcls && d->timg), DY_ERR_INVALID_ARG, "%s: null label pointer with n_labels %d", who, d->n_labels);
  DY_REQUIRE(d->n_labels == 0 || aligned16(d->tbox), DY_ERR_INVALID_ARG, "%s: tbox not 16-byte aligned", who);
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
  static const hipError_t attr_once = hipFuncSetAttribute((const void*)val_match_kernel_t<P>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)attr_once;
  hipLaunchKernelGGL(val_match_kernel_t<P>, dim3((unsigned)d->batch), dim3(VM_THREADS), vm_layout<P>(d->max_det).bytes,
                     reinterpret_cast<hipStream_t>(stream), a);
  return check_launch(kernel_name);
}

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_val_match(const dy_val_match_desc* d, dy_stream_t stream) {
  return launch_val_match<VmBox>(d, stream, "dy_val_match", "val_match_kernel");
}

extern "C" int32_t dy_val_match_rotated(const dy_val_match_rotated_desc* d, dy_stream_t stream) {
  return launch_val_match<VmRotated>(d, stream, "dy_val_match_rotated", "val_match_rotated_kernel");
}
