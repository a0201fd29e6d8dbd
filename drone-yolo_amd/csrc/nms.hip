// Batched NMS for the single-label path of ops.non_max_suppression (utils/ops.py:181-332)
// including the greedy NMS of torchvision.ops.nms (call site ops.py:312).
//
//   K1 nms_filter_kernel   all (image, anchor) pairs in parallel: best class score and FIRST
//                          arg-max class (ops.py:290), keep score > conf (ops.py:250,291) and
//                          the optional class filter (ops.py:294-295); survivors are appended as 64-bit
//                          keys (detect_row.h, wave_append).  Ascending key order == descending score,
//                          ties by ascending anchor index == the stable descending sort torchvision's CPU
//                          kernel uses on candidates listed in anchor order (ops.py:269 keeps anchor order).
//   K2 nms_suppress_kernel one workgroup per image: bitonic sort of the keys (LDS when they
//                          fit, the global workspace otherwise), truncate to max_nms
//                          (ops.py:301-302), then wave 0 runs the exact greedy scan in chunks of
//                          64 candidates: every lane tests its candidate against the kept
//                          list (LDS), then the chunk is resolved in score order with
//                          ballot/shuffle.  The scan stops at max_det kept (ops.py:313), which is
//                          exact because greedy NMS never revisits a kept box.  Serves the images with
//                          more than NMS_SMALL_CAP candidates (the validator's conf 0.001, multi_label).
//   K2s nms_small_kernel   the same for images with at most NMS_SMALL_CAP candidates, in 256 threads and
//                          22 KB of LDS with the scan on four waves (nms_scan.h).
//
// IoU and box arithmetic follow the reference operation by operation in fp32 with
// contraction off, so that kept indices are bit-identical to the CPU path for identical
// inputs:  xyxy = xy -/+ wh/2 (ops.py:432-449); boxes + cls*max_wh (ops.py:305,311);
// area = (x2-x1)*(y2-y1); inter = max(0,xx2-xx1)*max(0,yy2-yy1);
// suppress iff inter / (area_i + area_j - inter) > iou_thres.
#include "detect_row.h"
#include "nms_scan.h"

#pragma clang fp contract(off)

namespace dy {

__global__ __launch_bounds__(256) void nms_filter_kernel(const NmsArgs p) {
  const int lane = threadIdx.x & 63;
  const long long total = (long long)p.batch * p.A;
  const long long nthreads = (long long)gridDim.x * 256;
  // every wave iterates the same number of times so the ballot below is well defined
  const long long iters = (total + nthreads - 1) / nthreads;
  for (long long it = 0; it < iters; ++it) {
    const long long idx = it * nthreads + (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = idx < total;
    const int b = in ? (int)(idx / p.A) : 0;
    const int a = in ? (int)(idx - (long long)b * p.A) : 0;
    bool pass = false;
    float best = 0.f;
    int bj = 0;
    if (in) {
      const float* s = p.pred + ((size_t)b * p.nch + 4) * (size_t)p.A + a;
      best = s[0];
      for (int c = 1; c < p.nc; ++c) {
        const float v = s[(size_t)c * p.A];
        if (v > best) {
          best = v;
          bj = c;
        }
      }
      pass = best > p.conf;
      if (pass && p.cmask) pass = p.cmask[bj] != 0;
    }
    // A wave's 64 consecutive (image, anchor) pairs may straddle images: peel one image per
    // round, that of the lowest lane that still has a survivor to append (the round's leader in wave_append).
    u64 todo = __ballot(pass);
    while (todo != 0ull) {
      const int bb = __shfl(b, __ffsll((long long)todo) - 1);
      todo &= ~wave_append<true>(p.counts, p.keys, p.P, lane, pass && b == bb, bb, (unsigned)a, best, p.cls + (size_t)bb * p.A + a, bj);
    }
  }
}

// multi_label (the validator's NMS, ops.py:286-288: `i, j = torch.where(cls > conf_thres)`): every (anchor, class) pair scored above conf
// is a candidate of its own.  Candidate order in the reference is row-major over (anchor, class), so the tie order of the stable
// descending sort is ascending anchor * nc + class: that number is the key's low word.
__global__ __launch_bounds__(256) void nms_filter_ml_kernel(const NmsArgs p) {
  const int lane = threadIdx.x & 63;
  const long long total = (long long)p.batch * p.A;
  const long long nthreads = (long long)gridDim.x * 256;
  const long long iters = (total + nthreads - 1) / nthreads;
  for (long long it = 0; it < iters; ++it) {
    const long long idx = it * nthreads + (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = idx < total;
    const int b = in ? (int)(idx / p.A) : 0;
    const int a = in ? (int)(idx - (long long)b * p.A) : 0;
    const float* s = p.pred + ((size_t)b * p.nch + 4) * (size_t)p.A + a;
    for (int c = 0; c < p.nc; ++c) {  // (wave-uniform trip count: the ballots below are well defined)
      const float v = in ? s[(size_t)c * p.A] : 0.f;
      bool pass = in && v > p.conf;
      if (pass && p.cmask) pass = p.cmask[c] != 0;
      u64 todo = __ballot(pass);
      while (todo != 0ull) {
        const int bb = __shfl(b, __ffsll((long long)todo) - 1);
        todo &= ~wave_append<false>(p.counts, p.keys, p.P, lane, pass && b == bb, bb, (unsigned)a * (unsigned)p.nc + (unsigned)c, v);
      }
    }
  }
}

__device__ __forceinline__ bool iou_gt(float ix1, float iy1, float ix2, float iy2, float iarea, float jx1, float jy1,
                                       float jx2, float jy2, float jarea, float thr) {
  const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1);
  const float xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
  const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  const float inter = w * h;
  const float ovr = inter / (iarea + jarea - inter);
  return ovr > thr;
}

// ---- K2s nms_small_kernel: images with at most NMS_SMALL_CAP candidates (what the predictor produces at conf 0.25) ----------------
// One workgroup of 256 threads (4 waves) per image and LDS by need: the keys of NMS_SMALL_CAP entries, the kept list, a 64 x 64
// suppression bit matrix and one verdict word per wave: 16,928 + 20 * max_det bytes (22,928 B at max_det 300), so that the convolution
// workgroups of another stream fit on the same CU.  Same order, same arithmetic, same outputs as nms_suppress_kernel below:
//   sort     bitonic in LDS, 256 threads over the P2 / 2 <= 1024 compare-exchange pairs of a pass;
//   scan     nms_greedy_scan on four waves (nms_scan.h) with the policy NmsSmallScan below.
// The count is known on the device only, so dy_nms launches both kernels and each returns at once for the images of the other.
constexpr int NMS_SMALL_CAP = 2048;
constexpr int NMS_SMALL_THREADS = 256;
constexpr int NMS_SMALL_WAVES = NMS_SMALL_THREADS / 64;
constexpr int NMS_SMALL_FIXED_LDS = NMS_SMALL_CAP * 8 + 64 * 8 + NMS_SMALL_WAVES * 8;  // keys, bit matrix, verdict words

static inline size_t nms_small_lds_bytes(int max_det) { return (size_t)NMS_SMALL_FIXED_LDS + (size_t)max_det * 20; }

struct NmsCand {  // what a lane fetches for its candidate
  float cx, cy, w, h, score;
  int anchor, cls;
};

// the candidate a key stands for: anchor (and class, with multi_label) from the low word, score from the high word, box from pred
__device__ __forceinline__ NmsCand nms_cand(const NmsArgs& p, const float* pr, int b, u64 key) {
  NmsCand c;
  c.anchor = (int)(unsigned)(key & 0xffffffffull);
  c.score = __uint_as_float(~(unsigned)(key >> 32));
  if (p.multi) {
    c.cls = c.anchor % p.nc;
    c.anchor = c.anchor / p.nc;
  } else {
    c.cls = (int)p.cls[(size_t)b * p.A + c.anchor];
  }
  c.cx = pr[c.anchor];
  c.cy = pr[(size_t)p.A + c.anchor];
  c.w = pr[(size_t)2 * p.A + c.anchor];
  c.h = pr[(size_t)3 * p.A + c.anchor];
  return c;
}

struct NmsBoxes {
  float x1, y1, x2, y2;  // the output row's xyxy (ops.py:432-449)
  ScanBox off;           // the same plus cls * max_wh (ops.py:305,311) and its area: what the IoU sees
};

__device__ __forceinline__ NmsBoxes nms_boxes(const NmsArgs& p, const NmsCand& c) {
  NmsBoxes r;
  const float hw = c.w / 2.f, hh = c.h / 2.f;
  r.x1 = c.cx - hw, r.y1 = c.cy - hh, r.x2 = c.cx + hw, r.y2 = c.cy + hh;
  const float off = p.agnostic ? 0.f : (float)c.cls * p.max_wh;
  r.off.x1 = r.x1 + off, r.off.y1 = r.y1 + off, r.off.x2 = r.x2 + off, r.off.y2 = r.y2 + off;
  r.off.area = (r.off.x2 - r.off.x1) * (r.off.y2 - r.off.y1);
  r.off.cls = 0;
  return r;
}

__device__ __forceinline__ void nms_store_row(const NmsArgs& p, float* outb, int b, int at, const NmsCand& c, const NmsBoxes& bx) {
  float* o = outb + (size_t)at * 6;
  o[0] = bx.x1;
  o[1] = bx.y1;
  o[2] = bx.x2;
  o[3] = bx.y2;
  o[4] = c.score;
  o[5] = (float)c.cls;
  if (p.out_index) p.out_index[(size_t)b * p.max_det + at] = c.anchor;
}

struct NmsSmallScan {  // nms_greedy_scan's policy: class-offset boxes, IoU, kept list = float4 boxes + areas
  const NmsArgs& p;
  const u64* skeys;
  const float* pr;
  float* outb;
  float4* kbox;  // [max_det] offset xyxy of the kept boxes
  float* kar;    // [max_det] their areas
  int b;
  typedef NmsCand Cand;
  __device__ __forceinline__ Cand fetch(int i, int n) const { return i < n ? nms_cand(p, pr, b, skeys[i]) : Cand{0.f, 0.f, 0.f, 0.f, 0.f, 0, 0}; }
  __device__ __forceinline__ ScanBox box(const Cand& c) const { return nms_boxes(p, c).off; }
  __device__ __forceinline__ bool suppresses(const ScanBox& k, const ScanBox& c) const {
    return iou_gt(k.x1, k.y1, k.x2, k.y2, k.area, c.x1, c.y1, c.x2, c.y2, c.area, p.iou);
  }
  __device__ __forceinline__ ScanBox kept(int k) const {
    const float4 kb = kbox[k];
    return ScanBox{kb.x, kb.y, kb.z, kb.w, kar[k], 0};
  }
  __device__ __forceinline__ void keep(int at, const Cand& c, const ScanBox& bx) const {
    kbox[at] = make_float4(bx.x1, bx.y1, bx.x2, bx.y2);
    kar[at] = bx.area;
    nms_store_row(p, outb, b, at, c, nms_boxes(p, c));
  }
};

__global__ __launch_bounds__(NMS_SMALL_THREADS) void nms_small_kernel(const NmsArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  const int b = blockIdx.x;
  int n = p.counts[b];
  if (n > p.cap) n = p.cap;
  if (n > NMS_SMALL_CAP) return;  // nms_suppress_kernel's image
  u64* skeys = reinterpret_cast<u64*>(dyn_smem);
  u64* rows = skeys + NMS_SMALL_CAP;  // [64]
  u64* verdict = rows + 64;           // [NMS_SMALL_WAVES]
  float4* kbox = reinterpret_cast<float4*>(dyn_smem + NMS_SMALL_FIXED_LDS);
  const int tid = threadIdx.x;
  const u64* gkeys = p.keys + (size_t)b * p.P;

  int P2 = 1;
  while (P2 < n) P2 <<= 1;
  for (int i = tid; i < P2; i += NMS_SMALL_THREADS) skeys[i] = i < n ? gkeys[i] : ~0ull;
  __syncthreads();
  nms_bitonic_sort<NMS_SMALL_THREADS>(skeys, P2, tid);

  float* outb = p.out + (size_t)b * p.max_det * 6;
  const NmsSmallScan pol{p, skeys, p.pred + (size_t)b * p.nch * (size_t)p.A, outb, kbox, reinterpret_cast<float*>(kbox + p.max_det), b};
  nms_greedy_scan<NMS_SMALL_WAVES>(pol, n < p.max_nms ? n : p.max_nms, p.max_det, rows, verdict, outb,
                                   p.out_index ? p.out_index + (size_t)b * p.max_det : nullptr, p.out_count + b);
}

__global__ __launch_bounds__(1024) void nms_suppress_kernel(const NmsArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  u64* skeys = reinterpret_cast<u64*>(dyn_smem);
  float* kept = reinterpret_cast<float*>(dyn_smem + (size_t)p.SL * 8);  // 5 arrays of max_det
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  int n = p.counts[b];
  if (n > p.cap) n = p.cap;
  if (n <= NMS_SMALL_CAP) return;  // nms_small_kernel's image
  u64* gkeys = p.keys + (size_t)b * p.P;

  int P2 = 1;
  while (P2 < n) P2 <<= 1;
  const bool in_lds = P2 <= p.SL;
  // the LDS and the global sort are separate instantiations on purpose (nms_core.h)
  if (in_lds) {
    for (int i = tid; i < P2; i += 1024) skeys[i] = i < n ? gkeys[i] : ~0ull;
    __syncthreads();
    if (n > 1) nms_bitonic_sort<1024>(skeys, P2, tid);
  } else {
    for (int i = n + tid; i < P2; i += 1024) gkeys[i] = ~0ull;
    __syncthreads();
    nms_bitonic_sort<1024>(gkeys, P2, tid);
  }
  if (tid >= 64) return;  // wave 0 runs the greedy scan

  const int lane = tid;
  const int nn = n < p.max_nms ? n : p.max_nms;
  float* kx1 = kept;
  float* ky1 = kept + p.max_det;
  float* kx2 = kept + 2 * p.max_det;
  float* ky2 = kept + 3 * p.max_det;
  float* kar = kept + 4 * p.max_det;
  const float* pr = p.pred + (size_t)b * p.nch * (size_t)p.A;
  float* outb = p.out + (size_t)b * p.max_det * 6;
  int nk = 0;
  for (int c0 = 0; c0 < nn && nk < p.max_det; c0 += 64) {
    const int i = c0 + lane;
    bool alive = i < nn;
    NmsCand c{0.f, 0.f, 0.f, 0.f, 0.f, 0, 0};
    NmsBoxes bx{0.f, 0.f, 0.f, 0.f, ScanBox{0.f, 0.f, 0.f, 0.f, 0.f, 0}};
    if (alive) {
      c = nms_cand(p, pr, b, in_lds ? skeys[i] : gkeys[i]);
      bx = nms_boxes(p, c);
      for (int k = 0; k < nk; ++k)
        if (iou_gt(kx1[k], ky1[k], kx2[k], ky2[k], kar[k], bx.off.x1, bx.off.y1, bx.off.x2, bx.off.y2, bx.off.area, p.iou)) {
          alive = false;
          break;
        }
    }
    const float ox1 = bx.off.x1, oy1 = bx.off.y1, ox2 = bx.off.x2, oy2 = bx.off.y2, area = bx.off.area;
    u64 am = __ballot(alive);
    while (am != 0ull) {
      const int t = __ffsll((long long)am) - 1;  // best surviving candidate of the chunk (wave-uniform)
      // t is uniform, so broadcast its box with v_readlane (SGPR result) rather than LDS-routed shuffles
      auto bcast = [&](float v) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), t)); };
      const float tx1 = bcast(ox1), ty1 = bcast(oy1), tx2 = bcast(ox2), ty2 = bcast(oy2), tar = bcast(area);
      if (lane == t) {
        kx1[nk] = ox1;
        ky1[nk] = oy1;
        kx2[nk] = ox2;
        ky2[nk] = oy2;
        kar[nk] = area;
        nms_store_row(p, outb, b, nk, c, bx);
        alive = false;
      }
      ++nk;
      if (nk >= p.max_det) break;
      if (alive && lane > t && iou_gt(tx1, ty1, tx2, ty2, tar, ox1, oy1, ox2, oy2, area, p.iou)) alive = false;
      am = __ballot(alive);
    }
  }
  for (int r = nk * 6 + lane; r < p.max_det * 6; r += 64) outb[r] = 0.f;
  if (p.out_index)
    for (int r = nk + lane; r < p.max_det; r += 64) p.out_index[(size_t)b * p.max_det + r] = -1;
  if (lane == 0) p.out_count[b] = nk;
}

// scale_boxes + clip_boxes on the kept rows (utils/ops.py:92-127, 335-354).
__global__ __launch_bounds__(256) void scale_boxes_kernel(float* __restrict__ boxes, const int* __restrict__ counts,
                                                          const float* __restrict__ params, int batch, int max_det) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= batch * max_det) return;
  const int b = idx / max_det, r = idx - b * max_det;
  if (r >= counts[b]) return;
  const float gain = params[b * 5], px = params[b * 5 + 1], py = params[b * 5 + 2];
  const float cw = params[b * 5 + 3], ch = params[b * 5 + 4];
  float* o = boxes + (size_t)idx * 6;
  o[0] = fminf(fmaxf((o[0] - px) / gain, 0.f), cw);
  o[1] = fminf(fmaxf((o[1] - py) / gain, 0.f), ch);
  o[2] = fminf(fmaxf((o[2] - px) / gain, 0.f), cw);
  o[3] = fminf(fmaxf((o[3] - py) / gain, 0.f), ch);
}

static inline int next_pow2(int v) { return nms_next_pow2(v); }
static inline size_t align_up(size_t v, size_t a) { return nms_align_up(v, a); }

int nms_args_from_desc(const dy_nms_desc* d, const char* who, int64_t ws_extra, NmsArgs* out) {
  DY_REQUIRE(d && d->pred && d->out && d->out_count && d->workspace, DY_ERR_INVALID_ARG, "%s: null pointer", who);
  DY_REQUIRE(d->batch > 0 && d->nc > 0 && d->anchors > 0 && d->n_extra >= 0, DY_ERR_INVALID_ARG, "%s: bad dims", who);
  DY_REQUIRE(d->nc <= 65535, DY_ERR_UNSUPPORTED, "%s: nc %d > 65535", who, d->nc);
  DY_REQUIRE(d->conf_thres >= 0.f && d->conf_thres <= 1.f && d->iou_thres >= 0.f && d->iou_thres <= 1.f,
             DY_ERR_INVALID_ARG, "%s: thresholds must be in [0,1] (utils/ops.py:233-234)", who);
  DY_REQUIRE(d->max_det >= 1 && d->max_det <= 4096 && d->max_nms >= 1, DY_ERR_INVALID_ARG, "%s: max_det must be in [1,4096]", who);
  const bool multi = d->multi_label != 0 && d->nc > 1;  // (ops.py:255: multi_label &= nc > 1)
  DY_REQUIRE(!multi || (long long)d->anchors * d->nc < (1ll << 30), DY_ERR_UNSUPPORTED, "%s: multi_label with anchors * nc >= 2^30", who);
  DY_REQUIRE(!(multi && d->prefiltered), DY_ERR_UNSUPPORTED, "%s: the fused candidate filter is single-label; multi_label filters here", who);
  const int wcap = multi ? d->anchors * d->nc : d->anchors;
  const int64_t ws_need = (int64_t)nms_ws_bytes(d->batch, wcap) + ws_extra;
  DY_REQUIRE(d->workspace_bytes >= ws_need, DY_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)d->workspace_bytes,
             (long long)ws_need);
  DY_REQUIRE(aligned16(d->workspace), DY_ERR_INVALID_ARG, "%s: workspace not 16-byte aligned", who);

  NmsArgs a{};
  a.pred = d->pred;
  a.batch = d->batch;
  a.nc = d->nc;
  a.nch = 4 + d->nc + d->n_extra;
  a.A = d->anchors;
  a.conf = d->conf_thres;
  a.iou = d->iou_thres;
  a.max_det = d->max_det;
  a.max_nms = d->max_nms;
  a.max_wh = d->max_wh;
  a.agnostic = d->agnostic;
  a.cmask = d->classes_mask;
  a.out = d->out;
  a.out_count = d->out_count;
  a.out_index = d->out_index;
  const NmsWs w = nms_ws_layout(d->workspace, d->batch, wcap);
  a.multi = multi ? 1 : 0;
  a.cap = wcap;
  a.P = w.P;
  a.counts = w.counts;
  a.keys = reinterpret_cast<u64*>(w.keys);
  a.cls = w.cls;
  a.SL = a.P < 16384 ? a.P : 16384;
  *out = a;
  return DY_OK;
}

int nms_launch_filter(const NmsArgs& a, bool prefiltered, hipStream_t st) {
  if (prefiltered) return DY_OK;
  zero_async(a.counts, (size_t)a.batch * 4, st);
  const long long total = (long long)a.batch * a.A;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (a.multi) hipLaunchKernelGGL(nms_filter_ml_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(nms_filter_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return check_launch(a.multi ? "nms_filter_ml_kernel" : "nms_filter_kernel");
}

}  // namespace dy

using namespace dy;

extern "C" int64_t dy_nms_workspace_bytes(int32_t batch, int32_t anchors) {
  if (batch <= 0 || anchors <= 0) return -1;
  return (int64_t)nms_ws_bytes(batch, anchors);
}

extern "C" int32_t dy_nms(const dy_nms_desc* d, dy_stream_t stream) {
  NmsArgs a{};
  const int rc0 = nms_args_from_desc(d, "dy_nms", 0, &a);
  if (rc0 != DY_OK) return rc0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int wcap = a.cap;
  const int rcf = nms_launch_filter(a, d->prefiltered != 0, st);
  if (rcf != DY_OK) return rcf;
  // Both suppress kernels are launched: which of them an image belongs to (at most NMS_SMALL_CAP candidates or more) is known on
  // the device only, and the workgroups of the other kernel return in their first instructions.
  static const hipError_t attr_small = hipFuncSetAttribute((const void*)nms_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)attr_small;
  hipLaunchKernelGGL(nms_small_kernel, dim3((unsigned)d->batch), dim3(NMS_SMALL_THREADS), nms_small_lds_bytes(d->max_det), st, a);
  const int rc = check_launch("nms_small_kernel");
  if (rc != DY_OK) return rc;
  if (wcap <= NMS_SMALL_CAP) return DY_OK;  // no image can have more candidates
  const size_t smem = (size_t)a.SL * 8 + align_up((size_t)d->max_det * 5 * 4, 16);
  static const hipError_t attr_once = hipFuncSetAttribute((const void*)nms_suppress_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)attr_once;
  hipLaunchKernelGGL(nms_suppress_kernel, dim3((unsigned)d->batch), dim3(1024), smem, st, a);
  return check_launch("nms_suppress_kernel");
}

extern "C" int32_t dy_nms_small_cap(void) { return NMS_SMALL_CAP; }

extern "C" int32_t dy_scale_boxes(float* boxes, const int32_t* counts, const float* params, int32_t batch,
                                  int32_t max_det, dy_stream_t stream) {
  DY_REQUIRE(boxes && counts && params, DY_ERR_INVALID_ARG, "dy_scale_boxes: null pointer");
  DY_REQUIRE(batch > 0 && max_det > 0, DY_ERR_INVALID_ARG, "dy_scale_boxes: bad dims");
  const int total = batch * max_det;
  hipLaunchKernelGGL(scale_boxes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), boxes, counts, params, batch, max_det);
  return check_launch("scale_boxes_kernel");
}
