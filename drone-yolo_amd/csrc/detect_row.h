// The Detect decode of one anchor row and the NMS candidate append, once for every kernel that has them.
//
//   detect_decode_row   one lane, one anchor: its row of 4 * REG_MAX box bins + nc class logits (fp32, in LDS) ->
//                       DFL softmax expectation per side (block.py:58-76), dist2bbox in xywh at the anchor point (gx + 0.5, gy + 0.5)
//                       times the stride (utils/tal.py:333-357), sigmoid per class, and the best score with the FIRST arg-max class,
//                       as cls.max(1) (utils/ops.py:290).  Used by detect_decode_kernel (detect_decode.hip) and by detect_head_kernel /
//                       detect_head_split_kernel (detect_head.hip) behind their 1x1 convolutions.  Compiled with the library's
//                       contraction setting (on: num += e * i is one fma), so this header sets none.
//   wave_append         the candidate filter's append (utils/ops.py:250,291-295 decide `pass`): the lanes of a wave that pass, all of ONE
//                       image, take consecutive slots of that image's key list behind one atomicAdd of the lowest passing lane,
//                           key = (~float_bits(score) << 32) | low
//                       so that ascending key order is descending score, ties by ascending `low` (the anchor; anchor * nc + class for
//                       multi_label).  Used by the three kernels above and by the peeling loops of nms_filter_kernel /
//                       nms_filter_ml_kernel (nms.hip).  conv3x3_hhead.hip appends by hand, a tile late (Makefile, HHEAD_FLAGS).
//   FilterSink          where a fused filter appends and what it tests: the kernel-argument block of the four fused kernels, filled from
//                       a dy_nms workspace (nms_ws.h) by filter_sink_from_workspace.
#pragma once
#include "common_hip.h"
#include "nms_ws.h"

namespace DY_NS {

struct FilterSink {
  int* counts;               // [batch]
  unsigned long long* keys;  // [batch][P]; nullptr: no fused filter
  unsigned short* cls;       // [batch][A] best class of every candidate anchor
  int P;
  float conf;
  const uint8_t* cmask;  // [nc] or nullptr
};

// The checks of a fused filter's workspace and the sink it describes (`who` names the entry point in the error text).  The counts are
// NOT zeroed here: the decode entry points zero them before their launch, the Detect branch kernels rely on dy_nms_reset_counts.
static inline int filter_sink_from_workspace(const char* who, void* ws, int64_t ws_bytes, int batch, int anchors, int nc, float conf,
                                             const uint8_t* cmask, FilterSink* out) {
  DY_REQUIRE(nc <= 65535, DY_ERR_UNSUPPORTED, "%s: nc %d > 65535", who, nc);
  DY_REQUIRE(aligned16(ws) && ws_bytes >= (int64_t)nms_ws_bytes(batch, anchors), DY_ERR_WORKSPACE,
             "%s: nms_workspace too small or misaligned (need %lld bytes)", who, (long long)nms_ws_bytes(batch, anchors));
  const NmsWs w = nms_ws_layout(ws, batch, anchors);
  *out = FilterSink{w.counts, w.keys, w.cls, w.P, conf, cmask};
  return DY_OK;
}

struct RowBest {
  float best;  // highest class probability of the row
  int bj;      // its first arg-max
};

// r: the lane's row in LDS (16-byte aligned), class logits at r + cls_off; out: the image's (4 + nc, A) output, a: the anchor's column.
template <int REG_MAX>
__device__ __forceinline__ RowBest detect_decode_row(const float* r, int cls_off, int gx, int gy, float stride, float* out, int a, int A, int nc) {
  float dist[4];
#pragma unroll
  for (int side = 0; side < 4; ++side) {
    float v[REG_MAX];
#pragma unroll
    for (int i = 0; i < REG_MAX; i += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(r + side * REG_MAX + i);
      v[i] = t[0], v[i + 1] = t[1], v[i + 2] = t[2], v[i + 3] = t[3];
    }
    float mx = v[0];
#pragma unroll
    for (int i = 1; i < REG_MAX; ++i) mx = fmaxf(mx, v[i]);
    float den = 0.f, num = 0.f;
#pragma unroll
    for (int i = 0; i < REG_MAX; ++i) {
      const float e = __builtin_amdgcn_exp2f((v[i] - mx) * 1.4426950408889634f);
      den += e;
      num += e * (float)i;
    }
    dist[side] = num * __builtin_amdgcn_rcpf(den);
  }
  const float ax = (float)gx + 0.5f, ay = (float)gy + 0.5f;
  const float x1 = ax - dist[0], y1 = ay - dist[1], x2 = ax + dist[2], y2 = ay + dist[3];
  float* o = out + a;
  o[0] = (x1 + x2) * 0.5f * stride;
  o[(size_t)A] = (y1 + y2) * 0.5f * stride;
  o[(size_t)2 * A] = (x2 - x1) * stride;
  o[(size_t)3 * A] = (y2 - y1) * stride;
  const float* cl = r + cls_off;
  RowBest rb{0.f, 0};
  for (int c = 0; c < nc; ++c) {
    const float pr = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(cl[c] * -1.4426950408889634f));
    o[(size_t)(4 + c) * A] = pr;
    if (c == 0 || pr > rb.best) {  // first arg-max, as cls.max(1) (ops.py:290)
      rb.best = pr;
      rb.bj = c;
    }
  }
  return rb;
}

// Every lane of the wave calls it; `b` (the image) is the same on every lane that passes.  WITH_CLS: the lane's class goes to *cls_slot
// (multi_label keeps the class in the key and stores none).  Returns the ballot of `pass`.
template <bool WITH_CLS>
__device__ __forceinline__ unsigned long long wave_append(int* counts, unsigned long long* keys, int P, int lane, bool pass, int b, unsigned low,
                                                          float score, unsigned short* cls_slot = nullptr, int cls = 0) {
  const unsigned long long m = __ballot(pass);
  if (m != 0ull) {
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counts + b, __popcll(m));
    base = __shfl(base, leader);
    if (pass) {
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      keys[(size_t)b * P + pos] = ((unsigned long long)(~__float_as_uint(score)) << 32) | (unsigned long long)low;
      if constexpr (WITH_CLS) *cls_slot = (unsigned short)cls;
    }
  }
  return m;
}

// The fused filter behind detect_decode_row: the anchor passes with a best score above conf and its class in the mask.
__device__ __forceinline__ void filter_append(const FilterSink& f, int lane, bool valid, const RowBest& rb, int b, int a, int A) {
  bool pass = valid && rb.best > f.conf;
  if (pass && f.cmask) pass = f.cmask[rb.bj] != 0;
  wave_append<true>(f.counts, f.keys, f.P, lane, pass, b, (unsigned)a, rb.best, f.cls + (size_t)b * A + a, rb.bj);
}

}  // namespace DY_NS
