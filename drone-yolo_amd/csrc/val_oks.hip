// Pose validation matching on the padded NMS output, for a whole batch in one launch: BaseValidator.match_predictions on
// kpt_iou(gt_kpts, pred_kpts, sigma, area) (utils/metrics.py:156-175; PoseValidator._process_batch, models/yolo/pose/val.py), with the clip of
// its _prepare_pred (ops.scale_coords at gain 1 / pad 0 = clip_coords).  The pair score does not fit val_match.hip's VmItem (one float4 and one
// float per label or detection): a pose label is nkpt points, a visibility mask and an area.  The match rule is val_match.hip's:
//     best(d) = argmax_l m(l, d),  biou(d) = max_l m(l, d),   m(l, d) = oks(l, d) if tcls[l] == cls[d] else 0,  l over the image's labels
//     correct(d, t)  <=>  biou(d) >= t  and no d' < d has best(d') == best(d) and biou(d') >= t          (val_scan.h)
// with exact ties to the lower position in tbox and a NaN never the best.
//
//   val_oks_kernel_t  one workgroup (512 threads) per image.  The batch's labels are streamed in steps of OKS_STEP: a thread looks at the
//                     image index of its label and appends the ones of this image to an LDS stage: per keypoint one float4 (x, y, den,
//                     mask), per label its class, position in tbox and 1-norm of the mask.  den[k] and the mask are computed once per label
//                     of the image, not once per pair.  Then every thread runs its detections (tid, tid + 512, ...) over the stage with
//                     broadcast reads (every lane reads the same entry).  The per-detection LDS is class, biou, best and prev (16 B): the
//                     keypoints of 4096 detections (34 floats each at 17 keypoints) do not fit a CU's 160 KB.
//                     NK = 17 (the COCO skeleton): the detection's clipped coordinates sit in 34 registers for the whole step, loaded once
//                     per (detection, step) -- the pair loop is then LDS reads and VALU only.  NK = 0: any nkpt up to DY_OKS_MAX_KPT; the
//                     coordinates are re-read per pair from the L2-resident prediction tensor (34 floats of a detection are 34 lines in the
//                     dense form; a runtime-indexed register array would go to scratch).  The two instances run the same operations in the
//                     same order: their results are bit-equal.
//
// fp32, kpt_iou's order of operations, contraction off, correctly rounded divisions:
//     area = ((x2 - x1) * (y2 - y1)) * 0.53f;  den[k] = (((2 s[k]) * (2 s[k])) * (area + 1e-7f)) * 2
//     d[k] = dx * dx + dy * dy;  e[k] = d[k] / den[k];  oks = (sum_k expf(-e[k]) * mask[k]) / (n_visible + 1e-7f)
// expf is the device's and the sum runs k = 0, 1, ... in sequence (the host's is vectorised): tp equals the host's for inputs the reference
// decides with a margin (tools/make_poseval_golden.py).
#include "common_hip.h"
#include "val_scan.h"

#pragma clang fp contract(off)

namespace dy {

constexpr int OKS_THREADS = 512;  // one detection per thread at the validator's max_det 300
constexpr int OKS_MAX_IOUV = 16;
constexpr int OKS_MAX_DET = 4096;  // dy_nms's bound
constexpr int OKS_STEP = 64;       // labels looked at per step = capacity of the stage: 64 * 32 keypoints * 16 B = 32 KB at the cap
static_assert(DY_OKS_MAX_KPT == 32, "the stage is sized for DY_OKS_MAX_KPT");

struct ValOksArgs {
  const float* rows;
  const int* counts;
  const float* kpts;
  const int* index;
  long long stride_b, stride_ch, stride_d;
  int anchors;
  const float* tbox;
  const float* tkpt;
  const float* tcls;
  const int* timg;
  int batch, max_det, n_labels, n_iouv, nkpt, ndim;
  float clip_w, clip_h;
  int single_cls;
  float sigma[DY_OKS_MAX_KPT];
  float iouv[OKS_MAX_IOUV];
  uint8_t* tp;
  float* best_iou;
  int* best_label;
};

// The dynamic LDS of one workgroup, as byte offsets: the kernel's pointers and the host's request both come from here.
// max_det 4096 at 32 keypoints: 32 KB + 1 KB + 64 KB + 80 B = 97.1 KB.
struct OksLayout {
  unsigned lk;        // float4 [OKS_STEP * nkpt] the stage: x, y, den, mask (0 / 1) per keypoint of this image's labels of the current step
  unsigned lmeta;     // float4 [OKS_STEP]        the stage: class, position in tbox (int bits), n_visible + 1e-7f, unused
  unsigned dcls;      // float  [max_det]
  unsigned biou;      // float  [max_det]
  unsigned best;      // int    [max_det]
  unsigned prev;      // float  [max_det] val_rank_scan's scratch
  unsigned n_staged;  // int, padded to 16 B: labels staged so far, all steps together (never reset)
  unsigned thr;       // float  [OKS_MAX_IOUV] the thresholds
  unsigned bytes;
};

__host__ __device__ inline OksLayout oks_layout(int max_det, int nkpt) {
  const unsigned md = (unsigned)max_det;
  OksLayout o;
  o.lk = 0;
  o.lmeta = o.lk + OKS_STEP * (unsigned)nkpt * 16;
  o.dcls = o.lmeta + OKS_STEP * 16;
  o.biou = o.dcls + md * 4;
  o.best = o.biou + md * 4;
  o.prev = o.best + md * 4;
  o.n_staged = o.prev + md * 4;
  o.thr = o.n_staged + 16;
  o.bytes = o.thr + OKS_MAX_IOUV * 4;
  return o;
}

// the clip of _prepare_pred (ops.clip_coords): min(max(x, 0), w)
__device__ __forceinline__ float oks_clip(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }

// one keypoint's term of the sum: expf(-(d / den)) * mask
__device__ __forceinline__ float oks_term(const float4& s, float px, float py) {
  const float dx = s.x - px;
  const float dy = s.y - py;
  const float d = dx * dx + dy * dy;
  const float e = __fdiv_rn(d, s.z);
  return expf(-e) * s.w;
}

template <int NK>
__global__ __launch_bounds__(OKS_THREADS) void val_oks_kernel_t(const ValOksArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  const int nkpt = NK ? NK : p.nkpt;
  const OksLayout at = oks_layout(p.max_det, nkpt);
  float4* lk = reinterpret_cast<float4*>(dyn_smem + at.lk);
  float4* lmeta = reinterpret_cast<float4*>(dyn_smem + at.lmeta);
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

  const float* rb = p.rows + (size_t)b * p.max_det * 6;
  for (int d = tid; d < cnt; d += OKS_THREADS) {
    dcls[d] = p.single_cls ? 0.f : rb[(size_t)d * 6 + 5];
    biou[d] = -1.f;  // below every m: the first label of the image always takes an empty slot (a NaN m does not)
    best[d] = -1;
  }
  if (tid == 0) *n_staged = 0;
#pragma unroll
  for (int i = 0; i < OKS_MAX_IOUV; ++i)
    if (tid == i) thr[i] = p.iouv[i];
  __syncthreads();

  const float* kb = p.kpts + (long long)b * p.stride_b;
  const long long step_k = (long long)p.ndim * p.stride_ch;  // from one keypoint's x to the next one's
  int seen = 0;  // the counter after the previous step
  for (int l0 = 0; l0 < p.n_labels && cnt > 0; l0 += OKS_STEP) {  // (cnt is the same on every thread: the barriers are uniform)
    const int l = l0 + tid;
    if (tid < OKS_STEP && l < p.n_labels && p.timg[l] == b) {
      const int slot = atomicAdd(n_staged, 1) - seen;  // the stage is unordered; the tie rule below restores tbox order
      const float4 t = reinterpret_cast<const float4*>(p.tbox)[l];
      const float wh = (t.z - t.x) * (t.w - t.y);
      const float area = wh * 0.53f;
      const float ae = area + 1e-7f;
      const float* tk = p.tkpt + (size_t)l * nkpt * 3;
      float4* sk = lk + slot * nkpt;
      int nvis = 0;
      for (int k = 0; k < nkpt; ++k) {
        const float s2 = 2.f * p.sigma[k];
        const float den = ((s2 * s2) * ae) * 2.f;
        const bool vis = tk[3 * k + 2] != 0.f;
        nvis += vis ? 1 : 0;
        sk[k] = make_float4(tk[3 * k], tk[3 * k + 1], den, vis ? 1.f : 0.f);
      }
      lmeta[slot] = make_float4(p.tcls[l], __int_as_float(l), (float)nvis + 1e-7f, 0.f);
    }
    __syncthreads();
    const int ns = *n_staged - seen;  // at most OKS_STEP: one entry per label looked at
    seen += ns;
    for (int d = tid; d < cnt && ns > 0; d += OKS_THREADS) {
      long long off = d;
      if (p.index) {
        int a = p.index[(size_t)b * p.max_det + d];
        a = a < 0 ? 0 : (a >= p.anchors ? p.anchors - 1 : a);
        off = a;
      }
      const float* kd = kb + off * p.stride_d;
      float px[NK ? NK : 1], py[NK ? NK : 1];
      if (NK) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          px[k] = oks_clip(kd[k * step_k], p.clip_w);
          py[k] = oks_clip(kd[k * step_k + p.stride_ch], p.clip_h);
        }
      }
      const float qc = dcls[d];
      float bi = biou[d];
      int bl = best[d];
      for (int j = 0; j < ns; ++j) {  // (every lane reads the same stage entries: LDS broadcasts)
        const float4 mt = lmeta[j];
        float m = 0.f;
        if (mt.x == qc) {
          const float4* sk = lk + j * nkpt;
          float sum = 0.f;
          if (NK) {
#pragma unroll
            for (int k = 0; k < NK; ++k) sum += oks_term(sk[k], px[k], py[k]);
          } else {
            for (int k = 0; k < nkpt; ++k)
              sum += oks_term(sk[k], oks_clip(kd[k * step_k], p.clip_w), oks_clip(kd[k * step_k + p.stride_ch], p.clip_h));
          }
          m = __fdiv_rn(sum, mt.z);
        }
        const int l = __float_as_int(mt.y);
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

  // the rank scan over d' < d and the stores (val_scan.h, shared with dy_val_match and dy_val_mask_match)
  val_rank_scan(best, biou, prev, thr, cnt, p.max_det, p.n_iouv, p.tp + (size_t)b * p.max_det * p.n_iouv,
                p.best_iou ? p.best_iou + (size_t)b * p.max_det : nullptr, p.best_label ? p.best_label + (size_t)b * p.max_det : nullptr, 0, tid, OKS_THREADS);
}

template <int NK>
static void launch_val_oks(const ValOksArgs& a, hipStream_t stream) {
  static const hipError_t attr_once = hipFuncSetAttribute((const void*)val_oks_kernel_t<NK>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)attr_once;
  hipLaunchKernelGGL(val_oks_kernel_t<NK>, dim3((unsigned)a.batch), dim3(OKS_THREADS), oks_layout(a.max_det, a.nkpt).bytes, stream, a);
}

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_val_oks_match(const dy_val_oks_match_desc* d, dy_stream_t stream) {
  const char* who = "dy_val_oks_match";
  DY_REQUIRE(d && d->rows && d->counts && d->kpts && d->tp, DY_ERR_INVALID_ARG, "%s: null pointer (rows / counts / kpts / tp)", who);
  DY_REQUIRE(d->batch > 0 && d->max_det > 0 && d->max_det <= OKS_MAX_DET, DY_ERR_INVALID_ARG,
             "%s: bad dims (batch %d, max_det %d; max_det must be in [1,%d])", who, d->batch, d->max_det, OKS_MAX_DET);
  DY_REQUIRE(d->n_iouv >= 1 && d->n_iouv <= OKS_MAX_IOUV && d->iouv, DY_ERR_INVALID_ARG, "%s: n_iouv %d must be in [1,%d] with iouv set", who,
             d->n_iouv, OKS_MAX_IOUV);
  DY_REQUIRE(d->ndim == 2 || d->ndim == 3, DY_ERR_INVALID_ARG, "%s: ndim %d must be 2 or 3", who, d->ndim);
  DY_REQUIRE(d->nkpt >= 1, DY_ERR_INVALID_ARG, "%s: nkpt %d < 1", who, d->nkpt);
  DY_REQUIRE(d->nkpt <= DY_OKS_MAX_KPT, DY_ERR_UNSUPPORTED, "%s: nkpt %d; at most %d keypoints are built (the LDS stage)", who, d->nkpt, DY_OKS_MAX_KPT);
  DY_REQUIRE(d->sigma, DY_ERR_INVALID_ARG, "%s: null sigma", who);
  DY_REQUIRE(d->stride_b >= 0 && d->stride_ch >= 1 && d->stride_d >= 1, DY_ERR_INVALID_ARG, "%s: bad keypoint strides (%lld, %lld, %lld)", who,
             (long long)d->stride_b, (long long)d->stride_ch, (long long)d->stride_d);
  DY_REQUIRE(!d->index || d->anchors >= 1, DY_ERR_INVALID_ARG, "%s: index given with anchors %d", who, d->anchors);
  DY_REQUIRE(d->n_labels >= 0, DY_ERR_INVALID_ARG, "%s: n_labels %d < 0", who, d->n_labels);
  DY_REQUIRE(d->n_labels == 0 || (d->tbox && d->tkpt && d->tcls && d->timg), DY_ERR_INVALID_ARG, "%s: null label pointer with n_labels %d", who,
             d->n_labels);
  DY_REQUIRE(d->n_labels == 0 || aligned16(d->tbox), DY_ERR_INVALID_ARG, "%s: tbox not 16-byte aligned", who);
  ValOksArgs a{};
  a.rows = d->rows;
  a.counts = d->counts;
  a.kpts = d->kpts;
  a.index = d->index;
  a.stride_b = d->stride_b;
  a.stride_ch = d->stride_ch;
  a.stride_d = d->stride_d;
  a.anchors = d->anchors;
  a.tbox = d->tbox;
  a.tkpt = d->tkpt;
  a.tcls = d->tcls;
  a.timg = d->timg;
  a.batch = d->batch;
  a.max_det = d->max_det;
  a.n_labels = d->n_labels;
  a.n_iouv = d->n_iouv;
  a.nkpt = d->nkpt;
  a.ndim = d->ndim;
  a.clip_w = d->clip_w;
  a.clip_h = d->clip_h;
  a.single_cls = d->single_cls;
  for (int i = 0; i < d->nkpt; ++i) a.sigma[i] = d->sigma[i];
  for (int i = 0; i < d->n_iouv; ++i) a.iouv[i] = d->iouv[i];
  a.tp = d->tp;
  a.best_iou = d->best_iou;
  a.best_label = d->best_label;
  if (d->nkpt == 17)
    launch_val_oks<17>(a, reinterpret_cast<hipStream_t>(stream));
  else
    launch_val_oks<0>(a, reinterpret_cast<hipStream_t>(stream));
  return check_launch("val_oks_kernel");
}
