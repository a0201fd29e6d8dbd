// Tiled inference for batches of frames: the slicer of F frames in one launch and the cross-tile merge of F frames in one launch.
//
//   tiles_batch_kernel  F frames (F, hf, wf, 3) uint8 -> (F * K, 3, th, tw) fp32 / 255, tile f * K + k cut at offsets[k] = (y, x).  A lane owns four
//                       consecutive x of one tile row: twelve source bytes in one load where the four pixels lie inside the frame, three float4
//                       stores (one per plane).  Values are those of tiles_kernel (preproc.hip): (float)byte / 255.0f, pad_value / 255.0f outside.
//   tile_merge_kernel   one workgroup per frame over the per-tile dy_nms outputs rows (F * K, max_det, 6) + counts (F * K):
//                         compact   the rows r < counts[tile] are appended (wave-aggregated, one LDS atomic per wave) as 64-bit keys
//                                       key = (~float_bits(score) << 32) | slot,   slot = k * max_det + r
//                                   so that ascending key order is descending score, ties by ascending slot;
//                         sort      bitonic, in LDS when the keys fit, in the workspace otherwise (two calls: see nms_core.h on flat accesses);
//                         scan      nms_greedy_scan on 16 waves (nms_scan.h) with the kernel's policy.
//                       The kernel is a template over that policy; there are three, one per entry point.  TmBase holds what they share: the
//                       keys, the frame's rows and outputs, the kept list in LDS (a float4, a fifth float and the class per row: 24 bytes),
//                       the head of a candidate (key -> slot, score, its tile's (ox, oy), its row), kept() and the store of a kept box
//                       (its LDS row, the output row as the policy writes it, its out_index slot).  A policy adds ROW / SCORE (the floats
//                       of a row, the score's column), KEEP_BYTES, TAIL (a fusion pass behind the scan), its Cand and the columns it reads,
//                       box(), suppresses() and the output row.  The host side is shared likewise:
//                       tm_check tests what the three descriptors have in common, tm_launch<Pol> fills the arguments they have in common.
//   TmScan              dy_tile_merge.  A box is the row's xyxy plus its tile's (ox, oy): one fp32 add of an integer-valued float.  Classes
//                       are compared as integers; nothing is added to the coordinates.  All arithmetic is fp32 with contraction off, the IoU
//                       in the expression order of nms.hip's iou_gt (the reference's), intersection over the smaller area for metric 1.
//   TmFuseScan          dy_tile_fuse: TmScan (the same kept rows, scores, classes and slots) and the sorted position of every kept row;
//                       behind the scan the kept row absorbs what it suppressed instead of dropping it (greedy non-maximum merging):
//                         init      kept row k: members = 1, accumulators = its own box (the scan also left its sorted position, kpos[k]);
//                         absorb    one thread per candidate j of the sorted list: a binary search of kpos gives the kept rows ahead of j
//                                   (a prefix of the kept list, j itself when it is kept); the FIRST of them whose own box suppresses j
//                                   absorbs it (a walk of eight rows per step, the predicate only for rows that intersect one of the wave's
//                                   candidates) -- integer atomics on the kept row's accumulators, so the result does not depend on order:
//                                     union  atomic min / max of an order-preserving map of the float bits (any sign);
//                                     wbf    64-bit adds of w = rint(score * 2^16) and w * rint(coord * 64);
//                         write     rows with two or more members get their fused box (wbf: X / S / 64 in float64), clamped to the frame.
//                       LDS: keys [SL] * 8 + 656 fixed + 28 bytes per kept row (float4 box, area, class, sorted position), sized by need at
//                       launch: 4,096 keys + 1,000 kept = 60 KB, at merge_max_det 4096 the kept list takes 112 KB and 4,096 keys the rest.
//                       The accumulators (40 bytes per kept row) do not fit beside that, so they lie in the workspace behind the keys; only
//                       this workgroup touches its frame's, with an agent-scope fence and a barrier between the phases.
//   TmrScan             dy_tile_merge_rotated: the merge for oriented boxes.  Rows are the 7 columns of dy_nms_rotated (x, y, w, h, theta,
//                       conf, cls).  A box is the covariance row of probiou.h (rnms_row of the centre plus (ox, oy), w, h, theta: sinf / cosf
//                       once per candidate of a chunk, never per pair) and the predicate rnms_probiou(kept, candidate) >= thr -- the one
//                       expression the per-tile NMS and the validator use.  ScanBox's five floats hold x, y, a, b, c, so the kept list stays
//                       24 bytes a row and TmScan's LDS budget holds.  The expression's second half runs only when a ballot finds a lane that
//                       can still be suppressed: of the kept row's class and not ruled out by its distance terms (tmr_far_bound; no verdict
//                       can change).
#include "nms_scan.h"
#include "probiou.h"
#include "tile_limits.h"

#pragma clang fp contract(off)

namespace dy {

// ---- slicer -------------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void tiles_batch_kernel(const uint8_t* __restrict__ src, const int* __restrict__ offs, float* __restrict__ dst, int frames, int k,
                                                          int hf, int wf, int th, int tw, int swap_rb, float pad) {
  const int qw = (tw + 3) >> 2;  // quads of four x per tile row
  const long long total = (long long)frames * k * th * qw;
  const size_t plane = (size_t)th * tw;
  const size_t frame_bytes = (size_t)hf * wf * 3;
  const float padv = pad / 255.0f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % qw) * 4;
    long long t = i / qw;
    const int y = (int)(t % th);
    const int tile = (int)(t / th);  // f * k + tile of the frame
    const int f = tile / k, kk = tile - f * k;
    const int sy = offs[2 * kk] + y, sx = offs[2 * kk + 1] + x;
    float c0[4], c1[4], c2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c0[j] = c1[j] = c2[j] = padv;
    if ((unsigned)sy < (unsigned)hf) {
      const uint8_t* q = src + (size_t)f * frame_bytes + ((size_t)sy * wf + sx) * 3;
      if (sx >= 0 && sx + 3 < wf) {  // the four pixels are twelve consecutive bytes of the frame
        uint8_t b[12];
        __builtin_memcpy(b, q, 12);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          c0[j] = (float)b[3 * j] / 255.0f;
          c1[j] = (float)b[3 * j + 1] / 255.0f;
          c2[j] = (float)b[3 * j + 2] / 255.0f;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((unsigned)(sx + j) < (unsigned)wf) {
            c0[j] = (float)q[3 * j] / 255.0f;
            c1[j] = (float)q[3 * j + 1] / 255.0f;
            c2[j] = (float)q[3 * j + 2] / 255.0f;
          }
      }
    }
    float* d = dst + (size_t)tile * 3 * plane + (size_t)y * tw + x;
    const float* first = swap_rb ? c2 : c0;
    const float* last = swap_rb ? c0 : c2;
    if (VEC) {  // tw % 4 == 0 and dst 16-byte aligned: every quad is one aligned float4 per plane
      *reinterpret_cast<float4*>(d) = make_float4(first[0], first[1], first[2], first[3]);
      *reinterpret_cast<float4*>(d + plane) = make_float4(c1[0], c1[1], c1[2], c1[3]);
      *reinterpret_cast<float4*>(d + 2 * plane) = make_float4(last[0], last[1], last[2], last[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < tw) {
          d[j] = first[j];
          d[plane + j] = c1[j];
          d[2 * plane + j] = last[j];
        }
    }
  }
}

// ---- merge --------------------------------------------------------------------------------------------------------------------------------
constexpr int TM_THREADS = 1024;
constexpr int TM_WAVES = TM_THREADS / 64;
constexpr int TM_MAX_LDS_KEYS = 16384;                  // 128 KiB of the CU's 160 KiB
constexpr int TM_FIXED_LDS = 64 * 8 + TM_WAVES * 8 + 16;  // bit matrix, verdict words, two counters
constexpr int TM_KEEP_BYTES = 24;                       // float4 box, area, class per kept row
constexpr int TM_FUSE_KEEP_BYTES = TM_KEEP_BYTES + 4;   // dy_tile_fuse: and its position in the sorted list
constexpr int TM_ACC_WORDS = 5;                         // dy_tile_fuse: 64-bit accumulators per kept row (wbf: S, X of x1 y1 x2 y2; union: 4 x 32 bits)
constexpr int TM_UNION = 1, TM_WBF = 2;                 // dy_tile_fuse_desc.mode
constexpr int TM_ABSORB_STEP = 8;                       // dy_tile_fuse: kept rows a candidate is tested against per step of its walk
constexpr int TM_WBF_MAX_SIDE = 32768;                  // wbf: members * 2^16 * (side * 64) stays below 2^53

struct TmArgs {
  const float* rows;
  const int* counts;
  const int* offs;
  float* out;
  int* out_count;
  int* out_index;
  u64* keys;  // [frames][P]
  int K, max_det, N, P, SL;
  float fw, fh, thr;
  int metric, agnostic, keep;  // metric: dy_tile_merge and dy_tile_fuse
  // dy_tile_fuse only
  int mode;
  int* out_members;
  u64* acc;  // [frames][keep][TM_ACC_WORDS]
  // dy_tile_merge_rotated only
  float far;  // tmr_far_bound(thr)
};

// What every merge policy holds and does alike.  RW: the floats of an input and of an output row.
template <int RW>
struct TmBase {
  const TmArgs& p;
  const u64* skeys;
  const u64* gkeys;
  const float* frows;
  float* outb;
  int* outi;
  float4* kbox;  // [keep]: the first four floats of a kept ScanBox
  float* k5;     // its fifth
  int* kcls;
  bool in_lds;
  // the head of candidate i < n of the sorted list: slot and score from its key, its tile's place (ox, oy) in the frame, its row
  struct Head {
    int slot;
    float score, ox, oy;
    const float* q;
  };
  __device__ __forceinline__ Head head(int i) const {
    const u64 key = in_lds ? skeys[i] : gkeys[i];
    const int slot = (int)(unsigned)(key & 0xffffffffull);
    const int tile = slot / p.max_det;
    const float oy = (float)p.offs[2 * tile], ox = (float)p.offs[2 * tile + 1];
    return Head{slot, __uint_as_float(~(unsigned)(key >> 32)), ox, oy, frows + (size_t)slot * RW};
  }
  __device__ __forceinline__ ScanBox kept(int k) const {
    const float4 kb = kbox[k];
    return ScanBox{kb.x, kb.y, kb.z, kb.w, k5[k], kcls[k]};
  }
  // kept box `at` of the LDS list, output row `at` as the policy's write_row(float*) fills it, and its out_index slot
  template <typename WriteRow>
  __device__ __forceinline__ void keep_box(int at, const ScanBox& bx, int slot, WriteRow write_row) const {
    kbox[at] = make_float4(bx.x1, bx.y1, bx.x2, bx.y2);
    k5[at] = bx.area;
    kcls[at] = bx.cls;
    write_row(outb + (size_t)at * RW);
    if (outi) outi[at] = slot;
  }
};

// the sort key of a candidate: ascending key order is descending score, ties by ascending slot (the compact pass, dy_tile_mask_owner)
__device__ __forceinline__ u64 tm_key(float score, int slot) { return ((u64)(~__float_as_uint(score)) << 32) | (u64)(unsigned)slot; }

struct TmCand {
  float x1, y1, x2, y2, score;
  int slot, cls;
};

// box i (kept) suppresses box j: same class unless agnostic, then the overlap measure against thr.  Scalars by value: every operand is
// read ahead of the &&, so the predicate stays branch-free and the kept-list loop that calls it unrolls.
__device__ __forceinline__ bool tm_suppresses(int metric, int agnostic, float thr, float ix1, float iy1, float ix2, float iy2, float iarea, int icls, float jx1,
                                              float jy1, float jx2, float jy2, float jarea, int jcls) {
  const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1);
  const float xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
  const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  const float inter = w * h;
  const float den = metric ? fminf(iarea, jarea) : (iarea + jarea - inter);
  const float ovr = inter / den;
  return (agnostic || icls == jcls) && ovr > thr;
}

struct TmScan : TmBase<6> {  // nms_greedy_scan's policy: frame-coordinate boxes, classes compared as integers, IoU or IoS, clamped rows
  static constexpr int ROW = 6, SCORE = 4, KEEP_BYTES = TM_KEEP_BYTES;
  static constexpr bool TAIL = false;
  typedef TmCand Cand;
  __device__ __forceinline__ TmScan(const TmBase<6>& b) : TmBase<6>(b) {}
  __device__ __forceinline__ Cand fetch(int i, int n) const {
    Cand c{0.f, 0.f, 0.f, 0.f, 0.f, 0, -1};
    if (i < n) {
      const Head h = head(i);
      c.slot = h.slot;
      c.score = h.score;
      c.x1 = h.q[0] + h.ox;
      c.y1 = h.q[1] + h.oy;
      c.x2 = h.q[2] + h.ox;
      c.y2 = h.q[3] + h.oy;
      c.cls = (int)h.q[5];
    }
    return c;
  }
  __device__ __forceinline__ ScanBox box(const Cand& c) const { return ScanBox{c.x1, c.y1, c.x2, c.y2, (c.x2 - c.x1) * (c.y2 - c.y1), c.cls}; }
  __device__ __forceinline__ bool suppresses(const ScanBox& i, const ScanBox& j) const {
    return tm_suppresses(p.metric, p.agnostic, p.thr, i.x1, i.y1, i.x2, i.y2, i.area, i.cls, j.x1, j.y1, j.x2, j.y2, j.area, j.cls);
  }
  __device__ __forceinline__ void keep(int at, const Cand& c, const ScanBox& bx) const {
    keep_box(at, bx, c.slot, [&](float* o) {
      o[0] = fminf(fmaxf(c.x1, 0.f), p.fw);
      o[1] = fminf(fmaxf(c.y1, 0.f), p.fh);
      o[2] = fminf(fmaxf(c.x2, 0.f), p.fw);
      o[3] = fminf(fmaxf(c.y2, 0.f), p.fh);
      o[4] = c.score;
      o[5] = (float)c.cls;
    });
  }
};

// ---- oriented boxes (dy_tile_merge_rotated) -----------------------------------------------------------------------------------------------
struct TmrCand {
  float x, y, w, h, th, score;  // the centre in frame coordinates
  int slot, cls;
};

// t12 = t1 + t2 of rnms_probiou above which a pair cannot reach thr, whatever the rest of the expression gives.  rnms_probiou >= thr
// needs bd <= B = -log(1 - (1 - thr)^2 + eps).  With det > 0 the logarithm's argument is at least eps, so t3 >= 0.5 * logf(1e-7f) > -8.06
// and bd >= t12 - 8.06; t12 > B + 9 therefore leaves bd > B + 0.94, i.e. 1 - exp(-bd) + eps above (1 - thr)^2 by 0.61 (1 - (1 - thr)^2):
// at least 1.2e-3 for thr >= 1e-3, four orders of magnitude above the fp32 rounding of expf, the subtraction and sqrtf (a bd beyond the clamp
// at 100 or a NaN does not suppress either).  Below thr = 1e-3 a far pair's ProbIoU of 0 or -1.2e-7 may still reach thr: no pre-test.
// tmr_distance_terms restates the first lines of rnms_probiou (the same operations in the same order, contraction off: the same bits, and
// the compiler shares them with the call that follows); it serves the bound only, the verdict is rnms_probiou's.
__device__ __forceinline__ float tmr_distance_terms(const RRow& r1, const RRow& r2, float* det_out) {
  const float eps = 1e-7f;
  const float sa = r1.a + r2.a, sb = r1.b + r2.b, sc = r1.c + r2.c;
  const float dy = r1.y - r2.y, dx = r1.x - r2.x;
  const float det = sa * sb - sc * sc;
  const float den = det + eps;
  const float t1 = ((sa * (dy * dy) + sb * (dx * dx)) / den) * 0.25f;
  const float t2 = (((sc * (r2.x - r1.x)) * dy) / den) * 0.5f;
  *det_out = det;
  return t1 + t2;
}

static inline float tmr_far_bound(float thr) {
  if (!(thr >= 1e-3f)) return INFINITY;
  const double keep = (1.0 - (double)thr) * (1.0 - (double)thr);
  return (float)(-log(1.0 - keep + 1e-7) + 9.0);
}

struct TmrScan : TmBase<7> {  // nms_greedy_scan's policy: ScanBox = {x, y, a, b, c, cls}, the covariance row of a frame-coordinate box and its class
  static constexpr int ROW = 7, SCORE = 5, KEEP_BYTES = TM_KEEP_BYTES;
  static constexpr bool TAIL = false;
  typedef TmrCand Cand;
  __device__ __forceinline__ TmrScan(const TmBase<7>& b) : TmBase<7>(b) {}
  __device__ __forceinline__ Cand fetch(int i, int n) const {
    Cand c{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, -1};
    if (i < n) {
      const Head h = head(i);
      c.slot = h.slot;
      c.score = h.score;
      c.x = h.q[0] + h.ox;
      c.y = h.q[1] + h.oy;
      c.w = h.q[2];
      c.h = h.q[3];
      c.th = h.q[4];
      c.cls = (int)h.q[6];
    }
    return c;
  }
  __device__ __forceinline__ ScanBox box(const Cand& c) const {  // once per candidate of a chunk: the only sinf / cosf of the scan
    const RRow r = rnms_row(c.x, c.y, c.w, c.h, c.th);
    return ScanBox{r.x, r.y, r.a, r.b, r.c, c.cls};
  }
  // row i (kept) suppresses row j: the class rule and rnms_probiou(i, j) >= thr, the kept row first; a NaN compares false and suppresses
  // nothing.  i is wave-uniform at both call sites of the scan (a kept row, a row of the chunk's matrix).  What follows the distance terms
  // (two square roots, a division, logf, expf) is issued only when some lane of the wave can still be suppressed: one of i's class (any
  // with agnostic) whose distance terms do not already rule it out (tmr_far_bound).  A lane that is skipped has the verdict false either way.
  __device__ __forceinline__ bool suppresses(const ScanBox& i, const ScanBox& j) const {
    const RRow ri{i.x1, i.y1, i.x2, i.y2, i.area}, rj{j.x1, j.y1, j.x2, j.y2, j.area};
    float det;
    const float t12 = tmr_distance_terms(ri, rj, &det);
    const bool open = (p.agnostic || i.cls == j.cls) && !(det > 0.f && t12 > p.far);
    if (__ballot(open) == 0ull) return false;
    return open && rnms_probiou(ri, rj) >= p.thr;
  }
  __device__ __forceinline__ void keep(int at, const Cand& c, const ScanBox& bx) const {
    keep_box(at, bx, c.slot, [&](float* o) {  // clip_boxes on an xywh row, as dy_scale_rboxes: x and w to [0, frame_w], y and h to [0, frame_h]
      o[0] = fminf(fmaxf(c.x, 0.f), p.fw);
      o[1] = fminf(fmaxf(c.y, 0.f), p.fh);
      o[2] = fminf(fmaxf(c.w, 0.f), p.fw);
      o[3] = fminf(fmaxf(c.h, 0.f), p.fh);
      o[4] = c.th;
      o[5] = c.score;
      o[6] = (float)c.cls;
    });
  }
};

// ---- fusion (dy_tile_fuse) ----------------------------------------------------------------------------------------------------------------
struct TmFuseCand : TmCand {
  int pos;  // place in the sorted list
};

struct TmFuseScan : TmScan {  // TmScan, and the sorted position of every kept row
  static constexpr int KEEP_BYTES = TM_FUSE_KEEP_BYTES;
  static constexpr bool TAIL = true;
  int* kpos;  // [keep], behind kcls
  typedef TmFuseCand Cand;
  __device__ __forceinline__ TmFuseScan(const TmBase<6>& b) : TmScan(b), kpos(b.kcls + b.p.keep) {}
  __device__ __forceinline__ Cand fetch(int i, int n) const {
    Cand c;
    static_cast<TmCand&>(c) = TmScan::fetch(i, n);
    c.pos = i;
    return c;
  }
  __device__ __forceinline__ void keep(int at, const Cand& c, const ScanBox& bx) const {
    TmScan::keep(at, c, bx);
    kpos[at] = c.pos;
  }
};

// float -> unsigned whose integer order is the float order (negative values included), and back
__device__ __forceinline__ unsigned tm_ord(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tm_unord(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__device__ __forceinline__ long long tm_wbf_weight(float score) { return (long long)rintf(score * 65536.f); }
__device__ __forceinline__ long long tm_wbf_coord(float v) { return (long long)rintf(v * 64.f); }

// between two phases that hand this frame's accumulators from plain stores to atomics or from atomics to loads, inside the workgroup
__device__ __forceinline__ void tm_phase_barrier() {
  __threadfence();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// Behind the scan, every thread of the workgroup: nk rows kept out of the n sorted candidates.
__device__ __forceinline__ void tm_fuse_tail(const TmArgs& p, const TmFuseScan& pol, int f, int n, int nk) {
  const int tid = threadIdx.x;
  u64* acc = p.acc + (size_t)f * p.keep * TM_ACC_WORDS;
  int* mem = p.out_members + (size_t)f * p.keep;
  float* outb = p.out + (size_t)f * p.keep * 6;

  // init: a kept row is its own first member
  for (int k = tid; k < p.keep; k += TM_THREADS) {
    mem[k] = k < nk ? 1 : 0;
    if (k >= nk) continue;
    const float4 b = pol.kbox[k];
    if (p.mode == TM_UNION) {
      unsigned* a = reinterpret_cast<unsigned*>(acc + (size_t)k * TM_ACC_WORDS);
      a[0] = tm_ord(b.x);
      a[1] = tm_ord(b.y);
      a[2] = tm_ord(b.z);
      a[3] = tm_ord(b.w);
    } else {
      const int at = pol.kpos[k];
      const u64 key = pol.in_lds ? pol.skeys[at] : pol.gkeys[at];
      const long long w = tm_wbf_weight(__uint_as_float(~(unsigned)(key >> 32)));
      u64* a = acc + (size_t)k * TM_ACC_WORDS;
      a[0] = (u64)w;
      a[1] = (u64)(w * tm_wbf_coord(b.x));
      a[2] = (u64)(w * tm_wbf_coord(b.y));
      a[3] = (u64)(w * tm_wbf_coord(b.z));
      a[4] = (u64)(w * tm_wbf_coord(b.w));
    }
  }
  tm_phase_barrier();

  // absorb: candidate j goes to the first kept row ahead of it in the sorted list whose own box suppresses it
  for (int j = tid; j < n; j += TM_THREADS) {
    int lo = 0, hi = nk;  // lo: the kept rows with kpos < j
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (pol.kpos[mid] < j) lo = mid + 1;
      else hi = mid;
    }
    if (lo < nk && pol.kpos[lo] == j) continue;  // kept itself
    const TmCand c = pol.TmScan::fetch(j, n);
    const ScanBox bx = pol.box(c);
    // eight kept rows per step, their LDS reads in flight together, the exit tested once per step (a row past the prefix repeats its last).
    // The predicate (a division) runs only where the boxes intersect at all: inter == 0 gives 0 / den > thr, false for every den and
    // thr >= 0, and a wave whose 64 candidates all miss the kept row -- most rows of the walk -- skips it.  inter is the predicate's own
    // w * h, so the verdict is the scan's.
    int own = lo;
    for (int k0 = 0; k0 < lo && own == lo; k0 += TM_ABSORB_STEP) {
#pragma unroll
      for (int u = TM_ABSORB_STEP - 1; u >= 0; --u) {
        const int k = min(k0 + u, lo - 1);
        const float4 kb = pol.kbox[k];
        const float w = fmaxf(0.f, fminf(kb.z, bx.x2) - fmaxf(kb.x, bx.x1)), h = fmaxf(0.f, fminf(kb.w, bx.y2) - fmaxf(kb.y, bx.y1));
        if (__ballot(w * h > 0.f) != 0ull && pol.suppresses(pol.kept(k), bx)) own = k;  // (the ballot of the active lanes: a uniform branch)
      }
    }
    if (own == lo) continue;  // behind the stop at merge_max_det and matching no kept row: dropped
    atomicAdd(mem + own, 1);
    if (p.mode == TM_UNION) {
      unsigned* a = reinterpret_cast<unsigned*>(acc + (size_t)own * TM_ACC_WORDS);
      atomicMin(a + 0, tm_ord(c.x1));
      atomicMin(a + 1, tm_ord(c.y1));
      atomicMax(a + 2, tm_ord(c.x2));
      atomicMax(a + 3, tm_ord(c.y2));
    } else {
      const long long w = tm_wbf_weight(c.score);
      u64* a = acc + (size_t)own * TM_ACC_WORDS;
      atomicAdd(a + 0, (u64)w);
      atomicAdd(a + 1, (u64)(w * tm_wbf_coord(c.x1)));
      atomicAdd(a + 2, (u64)(w * tm_wbf_coord(c.y1)));
      atomicAdd(a + 3, (u64)(w * tm_wbf_coord(c.x2)));
      atomicAdd(a + 4, (u64)(w * tm_wbf_coord(c.y2)));
    }
  }
  tm_phase_barrier();

  // write: the scan left every kept row with its own box; a row that absorbed something gets the fused one
  for (int k = tid; k < nk; k += TM_THREADS) {
    if (__hip_atomic_load(mem + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 2) continue;
    float v[4];
    if (p.mode == TM_UNION) {
      const unsigned* a = reinterpret_cast<const unsigned*>(acc + (size_t)k * TM_ACC_WORDS);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = tm_unord(__hip_atomic_load(a + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    } else {
      const u64* a = acc + (size_t)k * TM_ACC_WORDS;
      const long long s = (long long)__hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (s == 0) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const long long x = (long long)__hip_atomic_load(a + 1 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v[c] = (float)(((double)x / (double)s) * 0.015625);
      }
    }
    float* o = outb + (size_t)k * 6;
    o[0] = fminf(fmaxf(v[0], 0.f), p.fw);
    o[1] = fminf(fmaxf(v[1], 0.f), p.fh);
    o[2] = fminf(fmaxf(v[2], 0.f), p.fw);
    o[3] = fminf(fmaxf(v[3], 0.f), p.fh);
  }
}

// One instantiation per policy: TmScan (dy_tile_merge), TmFuseScan (dy_tile_fuse), TmrScan (dy_tile_merge_rotated).  The fusing merge is
// a kernel of its own and not a run-time mode of TmScan's: the suppress path is at 115 of its 128 VGPRs.
template <typename Pol>
__global__ __launch_bounds__(TM_THREADS) void tile_merge_kernel(const TmArgs p) {
  constexpr int ROW = Pol::ROW, SCORE = Pol::SCORE;
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  u64* skeys = reinterpret_cast<u64*>(dyn_smem);  // [SL]
  u64* mrows = skeys + p.SL;                      // [64]
  u64* verdict = mrows + 64;                      // [TM_WAVES]
  int* ctr = reinterpret_cast<int*>(verdict + TM_WAVES);  // candidates of the frame, append cursor
  float4* kbox = reinterpret_cast<float4*>(dyn_smem + (size_t)p.SL * 8 + TM_FIXED_LDS);  // [keep]
  float* k5 = reinterpret_cast<float*>(kbox + p.keep);
  int* kcls = reinterpret_cast<int*>(k5 + p.keep);
  const int f = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const float* frows = p.rows + (size_t)f * p.N * ROW;
  const int* fcounts = p.counts + (size_t)f * p.K;
  u64* gkeys = p.keys + (size_t)f * p.P;

  // how many candidates the frame has decides where they are sorted
  if (tid == 0) ctr[0] = ctr[1] = 0;
  __syncthreads();
  int part = 0;
  for (int t = tid; t < p.K; t += TM_THREADS) {
    const int c = fcounts[t];
    part += c < 0 ? 0 : (c > p.max_det ? p.max_det : c);
  }
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0 && part != 0) atomicAdd(&ctr[0], part);
  __syncthreads();
  const int n = ctr[0];
  int P2 = 1;
  while (P2 < n) P2 <<= 1;
  const bool in_lds = P2 <= p.SL;

  // compact: every wave runs the same number of rounds so that the ballot is well defined
  for (int j0 = 0; j0 < p.N; j0 += TM_THREADS) {
    const int j = j0 + tid;
    bool valid = false;
    float score = 0.f;
    if (j < p.N) {
      const int tile = j / p.max_det, r = j - tile * p.max_det;
      valid = r < fcounts[tile];
      if (valid) score = frows[(size_t)j * ROW + SCORE];
    }
    const u64 m = __ballot(valid);
    int base = 0;
    if (lane == 0 && m != 0ull) base = atomicAdd(&ctr[1], __popcll(m));
    base = __shfl(base, 0);
    if (valid) {
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      const u64 key = tm_key(score, j);
      if (in_lds) skeys[pos] = key;
      else gkeys[pos] = key;
    }
  }
  if (in_lds) {
    for (int i = n + tid; i < P2; i += TM_THREADS) skeys[i] = ~0ull;
  } else {
    for (int i = n + tid; i < P2; i += TM_THREADS) gkeys[i] = ~0ull;
  }
  __syncthreads();
  if (in_lds) nms_bitonic_sort<TM_THREADS>(skeys, P2, tid);
  else nms_bitonic_sort<TM_THREADS>(gkeys, P2, tid);

  float* outb = p.out + (size_t)f * p.keep * ROW;
  int* outi = p.out_index ? p.out_index + (size_t)f * p.keep : nullptr;
  const Pol pol(TmBase<ROW>{p, skeys, gkeys, frows, outb, outi, kbox, k5, kcls, in_lds});
  const int nk = nms_greedy_scan<TM_WAVES, ROW>(pol, n, p.keep, mrows, verdict, outb, outi, p.out_count + f);
  if constexpr (Pol::TAIL) tm_fuse_tail(p, pol, f, n, nk);
}

// ---- dy_tile_mask_owner ------------------------------------------------------------------------------------------------------
// One thread per slot j of a frame, brute force over the frame's kept rows in chunks of a workgroup's width staged in LDS (box, area, class
// and sort key of the kept row's own candidate -- what the scan kept in its list).  Kept row t owns j when it IS j (equal keys) or, with
// stitch, when it stands before j (smaller key) and tm_suppresses(t, j): tm_fuse_tail's absorb rule, the first such t.  A kept j meets no
// earlier kept row that suppresses it (the scan would have dropped it), so it reaches itself.
constexpr int TMO_THREADS = 256;

struct TmoArgs {
  const float* rows;
  const int* counts;
  const int* offs;
  const int* kidx;
  const int* kcnt;
  int* owner;
  int K, max_det, N, keep, metric, agnostic, stitch;
  float thr;
};

struct TmoBox {
  float x1, y1, x2, y2, area;
  int cls;
  u64 key;
};

// candidate `slot` of the frame whose rows are frows: TmScan's fetch() and box(), and the key of the compact pass
__device__ __forceinline__ TmoBox tmo_box(const TmoArgs& p, const float* frows, int slot) {
  const int tile = slot / p.max_det;
  const float oy = (float)p.offs[2 * tile], ox = (float)p.offs[2 * tile + 1];
  const float* q = frows + (size_t)slot * 6;
  TmoBox b;
  b.x1 = q[0] + ox;
  b.y1 = q[1] + oy;
  b.x2 = q[2] + ox;
  b.y2 = q[3] + oy;
  b.area = (b.x2 - b.x1) * (b.y2 - b.y1);
  b.cls = (int)q[5];
  b.key = tm_key(q[4], slot);
  return b;
}

__global__ __launch_bounds__(TMO_THREADS) void tile_mask_owner_kernel(const TmoArgs p) {
  __shared__ float4 sbox[TMO_THREADS];
  __shared__ float sarea[TMO_THREADS];
  __shared__ int scls[TMO_THREADS];
  __shared__ u64 skey[TMO_THREADS];
  const int f = blockIdx.y, tid = threadIdx.x;
  const int j = blockIdx.x * TMO_THREADS + tid;
  const float* frows = p.rows + (size_t)f * p.N * 6;
  const int* fcounts = p.counts + (size_t)f * p.K;
  const int* fkidx = p.kidx + (size_t)f * p.keep;
  const int nk = min(max(p.kcnt[f], 0), p.keep);
  bool valid = false;
  if (j < p.N) {
    const int tile = j / p.max_det;
    valid = j - tile * p.max_det < fcounts[tile];
  }
  TmoBox me{0.f, 0.f, 0.f, 0.f, 0.f, -1, 0ull};
  if (valid) me = tmo_box(p, frows, j);
  int own = -1;
  bool done = !valid;
  for (int t0 = 0; t0 < nk; t0 += TMO_THREADS) {
    const int t = t0 + tid;
    TmoBox kb{0.f, 0.f, 0.f, 0.f, 0.f, -2, ~0ull};  // a kept_index outside the frame's slots: before nothing, equal to nothing
    if (t < nk) {
      const int slot = fkidx[t];
      if (slot >= 0 && slot < p.N) kb = tmo_box(p, frows, slot);
    }
    sbox[tid] = make_float4(kb.x1, kb.y1, kb.x2, kb.y2);
    sarea[tid] = kb.area;
    scls[tid] = kb.cls;
    skey[tid] = kb.key;
    __syncthreads();
    const int lim = min(TMO_THREADS, nk - t0);
    if (!done) {
      for (int u = 0; u < lim; ++u) {
        const u64 ku = skey[u];
        if (ku == me.key) {
          own = t0 + u, done = true;
          break;
        }
        if (!p.stitch || ku > me.key) continue;
        const float4 b = sbox[u];
        if (tm_suppresses(p.metric, p.agnostic, p.thr, b.x, b.y, b.z, b.w, sarea[u], scls[u], me.x1, me.y1, me.x2, me.y2, me.area, me.cls)) {
          own = t0 + u, done = true;
          break;
        }
      }
    }
    if (__syncthreads_and(done)) break;  // (a barrier as well: the next chunk overwrites the LDS rows)
  }
  if (j < p.N) p.owner[(size_t)f * p.N + j] = own;
}

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_tiles_batch_u8_to_nchw_f32(const uint8_t* frames, const int32_t* offsets_yx, float* dst, int32_t f, int32_t k, int32_t hf, int32_t wf,
                                                 int32_t th, int32_t tw, int32_t swap_rb, float pad_value, dy_stream_t stream) {
  DY_REQUIRE(frames && offsets_yx && dst, DY_ERR_INVALID_ARG, "dy_tiles_batch_u8_to_nchw_f32: null pointer");
  DY_REQUIRE(f > 0 && k > 0 && hf > 0 && wf > 0 && th > 0 && tw > 0, DY_ERR_INVALID_ARG, "dy_tiles_batch_u8_to_nchw_f32: bad dims");
  DY_REQUIRE((long long)f * k <= 0x7fffffffll / 2, DY_ERR_INVALID_ARG, "dy_tiles_batch_u8_to_nchw_f32: frames * tiles too large");
  const long long total = (long long)f * k * th * ((tw + 3) / 4);
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (tw % 4 == 0 && aligned16(dst))
    hipLaunchKernelGGL(tiles_batch_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, frames, offsets_yx, dst, f, k, hf, wf, th, tw, swap_rb ? 1 : 0, pad_value);
  else
    hipLaunchKernelGGL(tiles_batch_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, frames, offsets_yx, dst, f, k, hf, wf, th, tw, swap_rb ? 1 : 0, pad_value);
  return check_launch("dy_tiles_batch_u8_to_nchw_f32");
}

extern "C" int64_t dy_tile_merge_workspace_bytes(int32_t frames, int32_t tiles, int32_t max_det) {
  if (frames <= 0 || tiles <= 0 || max_det <= 0 || (long long)tiles * max_det > TM_MAX_SLOTS) return -1;
  return (int64_t)frames * nms_next_pow2(tiles * max_det) * 8;
}

// What the three descriptors share, by the fields they name alike.  `need`: the entry point's workspace size; `own`: its further required
// pointers are set (`own_names`, as the message lists them).  What one entry point alone has (metric, mode, the wbf side limit) it checks itself.
template <typename Desc>
static int tm_check(const Desc* d, const char* who, int64_t need, bool own = true, const char* own_names = "") {
  DY_REQUIRE(d && d->rows && d->counts && d->offsets_yx && d->out && d->out_count && own && d->workspace, DY_ERR_INVALID_ARG,
             "%s: null pointer (rows / counts / offsets_yx / out / out_count / %sworkspace)", who, own_names);
  DY_REQUIRE(d->frames > 0 && d->tiles > 0 && d->max_det > 0 && d->nc > 0 && d->frame_h > 0 && d->frame_w > 0 && d->merge_max_det > 0, DY_ERR_INVALID_ARG,
             "%s: bad dims (frames %d, tiles %d, max_det %d, nc %d, frame %d x %d, merge_max_det %d)", who, d->frames, d->tiles, d->max_det, d->nc, d->frame_h,
             d->frame_w, d->merge_max_det);
  DY_REQUIRE(d->thr >= 0.f && d->thr <= 1.f, DY_ERR_INVALID_ARG, "%s: thr must be in [0,1]", who);
  DY_REQUIRE((long long)d->tiles * d->max_det <= TM_MAX_SLOTS, DY_ERR_UNSUPPORTED, "%s: tiles * max_det = %lld > %d", who, (long long)d->tiles * d->max_det,
             TM_MAX_SLOTS);
  DY_REQUIRE(d->merge_max_det <= TM_MAX_KEEP, DY_ERR_UNSUPPORTED, "%s: merge_max_det %d > %d", who, d->merge_max_det, TM_MAX_KEEP);
  DY_REQUIRE(d->workspace_bytes >= need, DY_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)d->workspace_bytes, (long long)need);
  DY_REQUIRE(aligned16(d->workspace), DY_ERR_INVALID_ARG, "%s: workspace not 16-byte aligned", who);
  return DY_OK;
}

// The kernel arguments a checked descriptor describes (the fields the three share; `a` holds what only the entry point's own has) and the launch.
template <typename Pol, typename Desc>
static int tm_launch(const Desc* d, TmArgs a, const char* who, dy_stream_t stream) {
  a.rows = d->rows;
  a.counts = d->counts;
  a.offs = d->offsets_yx;
  a.out = d->out;
  a.out_count = d->out_count;
  a.out_index = d->out_index;
  a.keys = reinterpret_cast<u64*>(d->workspace);
  a.K = d->tiles;
  a.max_det = d->max_det;
  a.N = d->tiles * d->max_det;
  a.P = nms_next_pow2(a.N);
  a.fw = (float)d->frame_w;
  a.fh = (float)d->frame_h;
  a.thr = d->thr;
  a.agnostic = d->agnostic ? 1 : 0;
  a.keep = d->merge_max_det;
  // LDS by need: the keys of every slot when they fit beside the kept list, the largest power of two that does otherwise
  const size_t rest = (size_t)TM_FIXED_LDS + nms_align_up((size_t)a.keep * Pol::KEEP_BYTES, 16);
  a.SL = a.P < TM_MAX_LDS_KEYS ? a.P : TM_MAX_LDS_KEYS;
  while ((size_t)a.SL * 8 + rest > 160 * 1024) a.SL >>= 1;
  const size_t smem = (size_t)a.SL * 8 + rest;
  static const hipError_t attr_once = hipFuncSetAttribute((const void*)tile_merge_kernel<Pol>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)attr_once;
  hipLaunchKernelGGL(tile_merge_kernel<Pol>, dim3((unsigned)d->frames), dim3(TM_THREADS), smem, reinterpret_cast<hipStream_t>(stream), a);
  return check_launch(who);
}

extern "C" int32_t dy_tile_merge(const dy_tile_merge_desc* d, dy_stream_t stream) {
  if (const int s = tm_check(d, "dy_tile_merge", d ? dy_tile_merge_workspace_bytes(d->frames, d->tiles, d->max_det) : 0)) return s;
  DY_REQUIRE(d->metric == 0 || d->metric == 1, DY_ERR_INVALID_ARG, "dy_tile_merge: metric %d (0 = IoU, 1 = IoS)", d->metric);
  TmArgs a{};
  a.metric = d->metric;
  return tm_launch<TmScan>(d, a, "dy_tile_merge", stream);
}

extern "C" int64_t dy_tile_fuse_workspace_bytes(int32_t frames, int32_t tiles, int32_t max_det, int32_t merge_max_det) {
  const int64_t keys = dy_tile_merge_workspace_bytes(frames, tiles, max_det);
  if (keys < 0 || merge_max_det <= 0 || merge_max_det > TM_MAX_KEEP) return -1;
  return keys + (int64_t)frames * merge_max_det * TM_ACC_WORDS * 8;
}

extern "C" int32_t dy_tile_fuse(const dy_tile_fuse_desc* d, dy_stream_t stream) {
  const int64_t need = d ? dy_tile_fuse_workspace_bytes(d->frames, d->tiles, d->max_det, d->merge_max_det) : 0;
  if (const int s = tm_check(d, "dy_tile_fuse", need, d && d->out_members, "out_members / ")) return s;
  DY_REQUIRE(d->metric == 0 || d->metric == 1, DY_ERR_INVALID_ARG, "dy_tile_fuse: metric %d (0 = IoU, 1 = IoS)", d->metric);
  DY_REQUIRE(d->mode == TM_UNION || d->mode == TM_WBF, DY_ERR_INVALID_ARG, "dy_tile_fuse: mode %d (1 = union, 2 = wbf; suppression is dy_tile_merge)", d->mode);
  DY_REQUIRE(d->mode != TM_WBF || (d->frame_h <= TM_WBF_MAX_SIDE && d->frame_w <= TM_WBF_MAX_SIDE), DY_ERR_UNSUPPORTED,
             "dy_tile_fuse: wbf on a frame of %d x %d, sides above %d are beyond its integer sums", d->frame_h, d->frame_w, TM_WBF_MAX_SIDE);
  TmArgs a{};
  a.metric = d->metric;
  a.mode = d->mode;
  a.out_members = d->out_members;
  a.acc = reinterpret_cast<u64*>(reinterpret_cast<unsigned char*>(d->workspace) + dy_tile_merge_workspace_bytes(d->frames, d->tiles, d->max_det));
  return tm_launch<TmFuseScan>(d, a, "dy_tile_fuse", stream);
}

extern "C" int64_t dy_tile_merge_rotated_workspace_bytes(int32_t frames, int32_t tiles, int32_t max_det) {
  return dy_tile_merge_workspace_bytes(frames, tiles, max_det);  // the keys; the kept list is LDS
}

extern "C" int32_t dy_tile_merge_rotated(const dy_tile_merge_rotated_desc* d, dy_stream_t stream) {
  if (const int s = tm_check(d, "dy_tile_merge_rotated", d ? dy_tile_merge_rotated_workspace_bytes(d->frames, d->tiles, d->max_det) : 0)) return s;
  TmArgs a{};
  a.far = tmr_far_bound(d->thr);
  return tm_launch<TmrScan>(d, a, "dy_tile_merge_rotated", stream);
}

extern "C" int32_t dy_tile_mask_owner(const dy_tile_mask_owner_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->rows && d->counts && d->offsets_yx && d->kept_index && d->kept_count && d->owner, DY_ERR_INVALID_ARG,
             "dy_tile_mask_owner: null pointer (rows / counts / offsets_yx / kept_index / kept_count / owner)");
  DY_REQUIRE(d->frames > 0 && d->tiles > 0 && d->max_det > 0 && d->merge_max_det > 0, DY_ERR_INVALID_ARG,
             "dy_tile_mask_owner: bad dims (frames %d, tiles %d, max_det %d, merge_max_det %d)", d->frames, d->tiles, d->max_det, d->merge_max_det);
  DY_REQUIRE(d->thr >= 0.f && d->thr <= 1.f, DY_ERR_INVALID_ARG, "dy_tile_mask_owner: thr must be in [0,1]");
  DY_REQUIRE(d->metric == 0 || d->metric == 1, DY_ERR_INVALID_ARG, "dy_tile_mask_owner: metric %d (0 = IoU, 1 = IoS)", d->metric);
  DY_REQUIRE((long long)d->tiles * d->max_det <= TM_MAX_SLOTS, DY_ERR_UNSUPPORTED, "dy_tile_mask_owner: tiles * max_det = %lld > %d",
             (long long)d->tiles * d->max_det, TM_MAX_SLOTS);
  DY_REQUIRE(d->merge_max_det <= TM_MAX_KEEP, DY_ERR_UNSUPPORTED, "dy_tile_mask_owner: merge_max_det %d > %d", d->merge_max_det, TM_MAX_KEEP);
  DY_REQUIRE(d->frames <= 65535, DY_ERR_UNSUPPORTED, "dy_tile_mask_owner: %d frames are beyond the launch grid", d->frames);
  TmoArgs a;
  a.rows = d->rows, a.counts = d->counts, a.offs = d->offsets_yx, a.kidx = d->kept_index, a.kcnt = d->kept_count, a.owner = d->owner;
  a.K = d->tiles, a.max_det = d->max_det, a.N = d->tiles * d->max_det, a.keep = d->merge_max_det;
  a.metric = d->metric, a.agnostic = d->agnostic ? 1 : 0, a.stitch = d->stitch ? 1 : 0, a.thr = d->thr;
  hipLaunchKernelGGL(tile_mask_owner_kernel, dim3((unsigned)((a.N + TMO_THREADS - 1) / TMO_THREADS), (unsigned)d->frames), dim3(TMO_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return check_launch("tile_mask_owner_kernel");
}
