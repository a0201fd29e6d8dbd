// The multi-wave greedy scan of nms_small_kernel (nms.hip, 4 waves) and tile_merge_kernel (tile_merge.hip, 16 waves), behind the key sort.
//
// The sorted candidates are taken in chunks of 64, held alike by all WAVES waves (lane = candidate).  Per chunk:
//   wave w tests the 64 candidates against the kept boxes w, w + WAVES, ... and publishes a ballot of the suppressed lanes (`verdict`);
//   wave w also computes rows 64 / WAVES * w ... of the chunk's 64 x 64 suppression bit matrix (row i, bit j: box i as the kept box
//   suppresses candidate j; box i reaches every lane through v_readlane, i being wave-uniform);
//   after ONE barrier every wave ORs the verdicts, takes row[lane] into a register and resolves the chunk in score order with bit
//   operations only (lowest live bit t is kept; live &= ~row[t]) -- the same on all waves, so no second exchange is needed;
//   wave 0 appends the kept boxes and writes their rows; a second barrier publishes the kept list to the next chunk.
// The next chunk's candidates are fetched while the current one is scanned.  The scan stops at max_keep kept (exact: greedy NMS never
// revisits a kept box); then the rows past the count are zeroed, their indices set to -1 and the count stored.
//
// tile_merge.hip's oriented-box merge runs the same scan with ScanBox holding a covariance row (x, y, a, b, c of probiou.h) in place of
// x1, y1, x2, y2, area, and output rows of 7 floats (ROW).
// What differs between the kernels is the Policy (a small struct of the kernel's pointers):
//   Cand                                    what a lane fetches for its candidate of a chunk
//   Cand fetch(int i, int n)                candidate i of the sorted list, zeros for i >= n
//   ScanBox box(const Cand&)                the box the predicate sees (cls unused where classes are offsets of the coordinates)
//   bool suppresses(kept, cand)             "kept box suppresses candidate": the box arithmetic lives with the policy, under its
//                                           source's `fp contract(off)`, in a function of scalars by value (iou_gt, tm_suppresses):
//                                           a member read behind an && makes the predicate a branch, and the kept-list loop
//                                           around it then no longer unrolls
//   ScanBox kept(int k)                     kept box k of the LDS list
//   void keep(int at, const Cand&, const ScanBox&)   wave 0: kept box `at` of the LDS list and output row `at`
#pragma once
#include "nms_core.h"

namespace dy {

struct ScanBox {
  float x1, y1, x2, y2, area;
  int cls;
};

// a value every lane holds alike, moved to scalar registers (the compiler cannot see that an LDS read is wave-uniform)
__device__ __forceinline__ u64 nms_uniform64(u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | (u64)lo;
}

// Every thread of the 64 * WAVES of the workgroup calls it, behind the barrier that ends the sort.  mrows [64] and verdict [WAVES] are
// LDS; outb / outi (or nullptr) / out_count: the image's max_keep output rows, their indices and its count.  Returns the count (alike on
// every thread; tile_merge.hip's fusion pass goes on from it).  ROW: the floats of an output row (6; the oriented-box merge's rows have 7).
template <int WAVES, int ROW = 6, typename Policy>
__device__ __forceinline__ int nms_greedy_scan(const Policy& pol, int n, int max_keep, u64* mrows, u64* verdict, float* outb, int* outi, int* out_count) {
  constexpr int THREADS = 64 * WAVES, ROWS = 64 / WAVES;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const u64 lane_bit = 1ull << lane;
  int nk = 0;
  typename Policy::Cand nxt = pol.fetch(lane, n);
  for (int c0 = 0; c0 < n && nk < max_keep; c0 += 64) {
    const typename Policy::Cand c = nxt;
    nxt = pol.fetch(c0 + 64 + lane, n);
    const bool in = c0 + lane < n;
    const ScanBox bx = pol.box(c);
    // this wave's share of the kept list
    bool sup = false;
    for (int k = wave; k < nk; k += WAVES) sup |= pol.suppresses(pol.kept(k), bx);
    const u64 sm = __ballot(sup);
    // this wave's rows of the chunk's suppression matrix
    u64 myrow = 0ull;
    for (int r = 0; r < ROWS; ++r) {
      const int i = wave * ROWS + r;  // wave-uniform: v_readlane
      auto bcast = [&](float v) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), i)); };
      const ScanBox bi{bcast(bx.x1), bcast(bx.y1), bcast(bx.x2), bcast(bx.y2), bcast(bx.area), __builtin_amdgcn_readlane(bx.cls, i)};
      const u64 m = __ballot(pol.suppresses(bi, bx));
      if (lane == r) myrow = m;
    }
    if (lane < ROWS) mrows[wave * ROWS + lane] = myrow;
    if (lane == 0) verdict[wave] = sm;
    __syncthreads();
    u64 dead = 0ull;
    for (int w = 0; w < WAVES; ++w) dead |= verdict[w];
    const u64 row = mrows[lane];
    const unsigned row_lo = (unsigned)row, row_hi = (unsigned)(row >> 32);
    u64 am = __ballot(in) & ~nms_uniform64(dead);  // candidates of the chunk that no earlier kept box suppresses
    u64 km = 0ull;                                 // those the chunk keeps
    int cnt = 0;
    while (am != 0ull) {
      const int t = __ffsll((long long)am) - 1;  // best live candidate of the chunk (wave-uniform)
      km |= 1ull << t;
      ++cnt;
      if (nk + cnt >= max_keep) break;
      const u64 rt = ((u64)(unsigned)__builtin_amdgcn_readlane((int)row_hi, t) << 32) | (u64)(unsigned)__builtin_amdgcn_readlane((int)row_lo, t);
      am &= ~(rt | (1ull << t));
    }
    if (wave == 0 && (km & lane_bit) != 0ull) pol.keep(nk + __popcll(km & (lane_bit - 1ull)), c, bx);
    nk += cnt;
    __syncthreads();  // the kept list is complete before the next chunk reads it; mrows / verdict may be rewritten
  }
  for (int r = nk * ROW + tid; r < max_keep * ROW; r += THREADS) outb[r] = 0.f;
  if (outi)
    for (int r = nk + tid; r < max_keep; r += THREADS) outi[r] = -1;
  if (tid == 0) *out_count = nk;
  return nk;
}

}  // namespace dy
