// Mask half of the segmentation validator on the padded dy_nms output (models/yolo/segment/val.py:84-88, 164-208 of the reference):
// ops.process_mask(upsample=False) of every kept row, the overlap label map expanded to one binary mask per label (resized to the proto
// grid when that is twice the map), utils/metrics.py::mask_iou, and BaseValidator.match_predictions on it; a whole batch, no mask stored.
//
// The label map gives every pixel to at most one label, so the (n_label x n_pred) matrix product of mask_iou is a histogram: for one
// prediction, inter[l] = number of its mask pixels whose map value is l + 1.  At ratio 2 the resized-and-thresholded ground truth is the
// 2 x 2 replication of the map (the nearest source pixel carries a bilinear weight >= 9/16 > 0.5), so the map is read at [y >> 1, x >> 1].
//
//   val_mask_area_kernel   one workgroup per image: histogram of the map in LDS -> area_gt (each map pixel counts ratio^2 proto pixels).
//   val_mask_iou_kernel    one workgroup per (kept row, image).  The 32 coefficients are workgroup-uniform; the threads walk the crop window
//                          (mask_crop.h: the bounds dy_process_mask uses, NaN-corner rule included), one 128-byte proto pixel and one 32-term
//                          dot product each; where v > 0 the pixel counts for the predicted area and for the LDS bin of its map value.
//                          Then the IoU against every label of the image and a workgroup argmax: best(d), biou(d) (§ val_match.hip).
//   val_mask_scan_kernel   one workgroup per image: the rank scan of val_scan.h over best / biou -> tp_m.
//
// All counts are integers below 2^24 (mh * mw <= 2^24 is required), exact in fp32, so
//     iou = inter / (((area_gt + area_pred) - inter) + 1e-7f)
// with every operation rounded on its own (contraction off, correctly rounded division) is bit-equal to mask_iou's fp32 value.  A label
// of another class is m = 0 exactly, as `iou * correct_class` makes it.  The one inexact step is the sign of the fp32 dot product near 0.
#include "common_hip.h"
#include "mask_crop.h"
#include "val_scan.h"

#pragma clang fp contract(off)

namespace dy {

constexpr int VMM_THREADS = 256;
constexpr int VMM_AREA_THREADS = 1024;
constexpr int VMM_SCAN_THREADS = 512;
constexpr int VMM_MAX_LABELS = 1024;  // labels per image: one 4-byte LDS bin each (+ the background bin)
constexpr int VMM_MAX_IOUV = 16;
constexpr int VMM_MAX_DET = 4096;  // dy_nms's bound; 12 bytes of LDS per row in the scan

struct ValMaskArgs {
  const float* protos;
  const float* side;
  const float* rows;
  const int* counts;
  const void* map;
  const float* tcls;
  const int* loff;
  int batch, max_det, mh, mw, ld_p, gh, gw, shift, map_i32, n_labels, l_cap, n_iouv;
  float ratio_x, ratio_y;
  int single_cls;
  float iouv[VMM_MAX_IOUV];
  uint8_t* tp_m;
  float* best_iou;
  int* best_label;
  int* area_gt;
  int* inter;
  int* area_pred;
};

// the image's slice of the labels, clamped into [0, n_labels] and to l_cap entries: first label and how many
__device__ __forceinline__ int2 vmm_labels(const ValMaskArgs& p, int b) {
  int lo = p.loff[b], hi = p.loff[b + 1];
  lo = min(max(lo, 0), p.n_labels);
  hi = min(max(hi, lo), p.n_labels);
  return make_int2(lo, min(hi - lo, p.l_cap));
}

__device__ __forceinline__ int vmm_map_at(const ValMaskArgs& p, long long i) {
  return p.map_i32 ? reinterpret_cast<const int*>(p.map)[i] : (int)reinterpret_cast<const unsigned char*>(p.map)[i];
}

__global__ __launch_bounds__(VMM_AREA_THREADS) void val_mask_area_kernel(const ValMaskArgs p) {
  __shared__ int hist[VMM_MAX_LABELS + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nl = vmm_labels(p, b).y;
  for (int i = tid; i <= nl; i += VMM_AREA_THREADS) hist[i] = 0;
  __syncthreads();
  const int px = p.gh * p.gw;  // <= mh * mw <= 2^24
  if (nl > 0)
    for (int i = tid; i < px; i += VMM_AREA_THREADS) {
      const int m = vmm_map_at(p, (long long)b * px + i);
      if (m >= 1 && m <= nl) atomicAdd(&hist[m], 1);
    }
  __syncthreads();
  for (int l = tid; l < p.l_cap; l += VMM_AREA_THREADS) p.area_gt[(long long)b * p.l_cap + l] = l < nl ? hist[l + 1] << (2 * p.shift) : 0;
}

__global__ __launch_bounds__(VMM_THREADS) void val_mask_iou_kernel(const ValMaskArgs p) {
  __shared__ int hist[VMM_MAX_LABELS + 1];
  __shared__ float red_m[VMM_THREADS];
  __shared__ int red_l[VMM_THREADS];
  __shared__ int area_s;
  const int d = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  int cnt = p.counts[b];
  cnt = cnt < 0 ? 0 : (cnt > p.max_det ? p.max_det : cnt);
  const long long row = (long long)b * p.max_det + d;
  if (d >= cnt) {  // (workgroup-uniform) no prediction in this row: its counts are zeros, the scan kernel writes the rest
    if (p.inter)
      for (int l = tid; l < p.l_cap; l += VMM_THREADS) p.inter[row * p.l_cap + l] = 0;
    if (p.area_pred && tid == 0) p.area_pred[row] = 0;
    return;
  }
  const int2 lab = vmm_labels(p, b);
  const int l0 = lab.x, nl = lab.y;
  for (int i = tid; i <= nl; i += VMM_THREADS) hist[i] = 0;
  if (tid == 0) area_s = 0;
  __syncthreads();

  const float* srow = p.side + row * 36;
  float cf[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) cf[k] = srow[4 + k];
  // ops.process_mask: the unscaled box times (mw / iw, mh / ih), then crop_mask on the proto grid
  const CropWin cw = crop_window(srow[0] * p.ratio_x, srow[1] * p.ratio_y, srow[2] * p.ratio_x, srow[3] * p.ratio_y, p.mw, p.mh);
  const int ww = cw.x_hi - cw.x_lo + 1, wh = cw.y_hi - cw.y_lo + 1;
  int mine = 0;
  if (ww > 0 && wh > 0) {
    const float* grid = p.protos + (long long)b * p.mh * p.mw * p.ld_p;
    const long long mbase = (long long)b * p.gh * p.gw;
    const int npx = ww * wh;  // <= mh * mw <= 2^24
    for (int i = tid; i < npx; i += VMM_THREADS) {
      const int yy = i / ww;
      const int y = cw.y_lo + yy, x = cw.x_lo + (i - yy * ww);
      const float v = proto_dot32(cf, grid + ((long long)y * p.mw + x) * p.ld_p);
      if (v > 0.f) {
        ++mine;
        if (nl > 0) {
          const int m = vmm_map_at(p, mbase + (long long)(y >> p.shift) * p.gw + (x >> p.shift));
          if (m >= 1 && m <= nl) atomicAdd(&hist[m], 1);
        }
      }
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((tid & (kWave - 1)) == 0 && mine) atomicAdd(&area_s, mine);
  __syncthreads();
  const int ap = area_s;
  if (p.area_pred && tid == 0) p.area_pred[row] = ap;

  const float dc = p.single_cls ? 0.f : p.rows[row * 6 + 5];
  const float fap = (float)ap;
  float bm = -1.f;  // below every m: the first label of the image always takes an empty slot
  int bl = -1;
  for (int l = tid; l < p.l_cap; l += VMM_THREADS) {
    const int in = l < nl ? hist[l + 1] : 0;
    if (p.inter) p.inter[row * p.l_cap + l] = in;
    if (l >= nl) continue;
    float m = 0.f;
    if (p.tcls[l0 + l] == dc) {
      const float fin = (float)in;
      const float sum = (float)p.area_gt[(long long)b * p.l_cap + l] + fap;
      const float uni = sum - fin;
      m = __fdiv_rn(fin, uni + 1e-7f);
    }
    if (m > bm) bm = m, bl = l;  // (l ascends inside a thread: an exact tie keeps the lower position)
  }
  red_m[tid] = bm;
  red_l[tid] = bl;
  __syncthreads();
  for (int s = VMM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const float om = red_m[tid + s];
      const int ol = red_l[tid + s];
      const float mm = red_m[tid];
      const int ml = red_l[tid];
      if (ol >= 0 && (ml < 0 || om > mm || (om == mm && ol < ml))) red_m[tid] = om, red_l[tid] = ol;
    }
    __syncthreads();
  }
  if (tid == 0) {  // the scan kernel reads these (position inside the image; -1: the image has no label)
    p.best_iou[row] = red_l[0] >= 0 ? red_m[0] : 0.f;
    p.best_label[row] = red_l[0];
  }
}

static inline size_t val_mask_scan_lds(int max_det) { return (size_t)max_det * 12 + VMM_MAX_IOUV * 4; }

__global__ __launch_bounds__(VMM_SCAN_THREADS) void val_mask_scan_kernel(const ValMaskArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  float* biou = reinterpret_cast<float*>(dyn_smem);          // [max_det]
  int* best = reinterpret_cast<int*>(biou + p.max_det);      // [max_det]
  float* prev = reinterpret_cast<float*>(best + p.max_det);  // [max_det]
  float* thr = prev + p.max_det;                             // [VMM_MAX_IOUV]
  const int b = blockIdx.x, tid = threadIdx.x;
  int cnt = p.counts[b];
  cnt = cnt < 0 ? 0 : (cnt > p.max_det ? p.max_det : cnt);
  const long long r0 = (long long)b * p.max_det;
  for (int d = tid; d < cnt; d += VMM_SCAN_THREADS) {
    biou[d] = p.best_iou[r0 + d];
    best[d] = p.best_label[r0 + d];
  }
#pragma unroll
  for (int i = 0; i < VMM_MAX_IOUV; ++i)
    if (tid == i) thr[i] = p.iouv[i];
  __syncthreads();
  // best_label leaves as the position in tcls, as dy_val_match's does
  val_rank_scan(best, biou, prev, thr, cnt, p.max_det, p.n_iouv, p.tp_m + (size_t)r0 * p.n_iouv, p.best_iou + r0, p.best_label + r0, vmm_labels(p, b).x,
                tid, VMM_SCAN_THREADS);
}

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_val_mask_match(const dy_val_mask_match_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->protos && d->side && d->rows && d->counts && d->loff && d->tp_m && d->best_iou && d->best_label && d->area_gt, DY_ERR_INVALID_ARG,
             "dy_val_mask_match: null pointer (protos / side / rows / counts / loff / tp_m / best_iou / best_label / area_gt)");
  DY_REQUIRE(d->nm == 32, DY_ERR_UNSUPPORTED, "dy_val_mask_match: built for nm = 32 mask coefficients");
  DY_REQUIRE(d->batch > 0 && d->batch <= 65535 && d->max_det > 0 && d->max_det <= VMM_MAX_DET, DY_ERR_INVALID_ARG,
             "dy_val_mask_match: bad dims (batch %d must be in [1,65535], max_det %d in [1,%d])", d->batch, d->max_det, VMM_MAX_DET);
  DY_REQUIRE(d->mh > 0 && d->mw > 0 && (long long)d->mh * d->mw <= (1ll << 24), DY_ERR_INVALID_ARG,
             "dy_val_mask_match: proto grid %d x %d must hold 1..2^24 pixels (the counts must be exact in fp32)", d->mh, d->mw);
  DY_REQUIRE(d->ld_p >= 32 && d->ld_p % 4 == 0 && aligned16(d->protos), DY_ERR_INVALID_ARG, "dy_val_mask_match: protos must be 16-byte aligned 128-byte rows");
  DY_REQUIRE(d->n_iouv >= 1 && d->n_iouv <= VMM_MAX_IOUV && d->iouv, DY_ERR_INVALID_ARG, "dy_val_mask_match: n_iouv %d must be in [1,%d] with iouv set",
             d->n_iouv, VMM_MAX_IOUV);
  DY_REQUIRE(d->in_w > 0 && d->in_h > 0, DY_ERR_INVALID_ARG, "dy_val_mask_match: bad input size %d x %d", d->in_w, d->in_h);
  DY_REQUIRE(d->n_labels >= 0 && d->l_cap >= 1, DY_ERR_INVALID_ARG, "dy_val_mask_match: n_labels %d < 0 or l_cap %d < 1", d->n_labels, d->l_cap);
  DY_REQUIRE(d->l_cap <= VMM_MAX_LABELS, DY_ERR_UNSUPPORTED, "dy_val_mask_match: l_cap %d: at most %d labels per image (one LDS bin each)", d->l_cap,
             VMM_MAX_LABELS);
  DY_REQUIRE(d->n_labels == 0 || (d->map && d->tcls), DY_ERR_INVALID_ARG, "dy_val_mask_match: null map / tcls with n_labels %d", d->n_labels);
  DY_REQUIRE(d->map_dtype == DY_MAP_U8 || d->map_dtype == DY_MAP_I32, DY_ERR_INVALID_ARG, "dy_val_mask_match: map_dtype %d is neither DY_MAP_U8 nor DY_MAP_I32",
             d->map_dtype);
  int shift = -1;
  if (d->gh == d->mh && d->gw == d->mw) shift = 0;
  if (d->gh > 0 && d->gw > 0 && 2 * d->gh == d->mh && 2 * d->gw == d->mw) shift = 1;
  DY_REQUIRE(shift >= 0, DY_ERR_INVALID_ARG, "dy_val_mask_match: proto grid %d x %d must equal the label map %d x %d or be exactly twice it on both axes",
             d->mh, d->mw, d->gh, d->gw);
  ValMaskArgs a{};
  a.protos = d->protos, a.side = d->side, a.rows = d->rows, a.counts = d->counts, a.map = d->map, a.tcls = d->tcls, a.loff = d->loff;
  a.batch = d->batch, a.max_det = d->max_det, a.mh = d->mh, a.mw = d->mw, a.ld_p = d->ld_p, a.gh = d->gh, a.gw = d->gw, a.shift = shift;
  a.map_i32 = d->map_dtype == DY_MAP_I32, a.n_labels = d->n_labels, a.l_cap = d->l_cap, a.n_iouv = d->n_iouv;
  a.ratio_x = (float)((double)d->mw / (double)d->in_w), a.ratio_y = (float)((double)d->mh / (double)d->in_h);
  a.single_cls = d->single_cls;
  for (int i = 0; i < d->n_iouv; ++i) a.iouv[i] = d->iouv[i];
  a.tp_m = d->tp_m, a.best_iou = d->best_iou, a.best_label = d->best_label, a.area_gt = d->area_gt, a.inter = d->inter, a.area_pred = d->area_pred;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(val_mask_area_kernel, dim3((unsigned)d->batch), dim3(VMM_AREA_THREADS), 0, s, a);
  int32_t rc = check_launch("val_mask_area_kernel");
  if (rc != DY_OK) return rc;
  hipLaunchKernelGGL(val_mask_iou_kernel, dim3((unsigned)d->max_det, (unsigned)d->batch), dim3(VMM_THREADS), 0, s, a);
  rc = check_launch("val_mask_iou_kernel");
  if (rc != DY_OK) return rc;
  hipLaunchKernelGGL(val_mask_scan_kernel, dim3((unsigned)d->batch), dim3(VMM_SCAN_THREADS), val_mask_scan_lds(d->max_det), s, a);
  return check_launch("val_mask_scan_kernel");
}
