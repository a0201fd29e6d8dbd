// The candidate stage dy_nms (nms.hip) and dy_nms_rotated (obb.hip) share: the kernel arguments, the filter launch and the key sort
// (tile_merge.hip sorts with it too).  The keys are those of detect_row.h's wave_append.
#pragma once
#include "common_hip.h"
#include "nms_ws.h"

namespace dy {

typedef unsigned long long u64;

struct NmsArgs {
  const float* pred;
  int batch, nc, nch, A;  // nch = 4 + nc + n_extra rows per image
  float conf, iou;
  int max_det, max_nms;
  float max_wh;
  int agnostic;
  const uint8_t* cmask;
  float* out;
  int* out_count;
  int* out_index;
  int* counts;          // [batch]
  u64* keys;            // [batch][P]
  unsigned short* cls;  // [batch][A] best class of every candidate anchor
  int P;                // per-image key capacity (power of two >= A)
  int SL;               // LDS sort capacity in keys (power of two)
  int multi;            // multi_label (ops.py:286-288): a candidate is an (anchor, class) pair, key low word = anchor * nc + class
  int cap;              // candidates an image can have: A, or A * nc with multi
};

// The checks of a dy_nms_desc both entry points make before any launch, and the kernel arguments it describes (`who` names the entry
// point in the error text; `ws_extra`: bytes it needs behind the dy_nms workspace).  Defined in nms.hip.
int nms_args_from_desc(const dy_nms_desc* d, const char* who, int64_t ws_extra, NmsArgs* a);
// Candidate stage: zero the counts and run the filter (nms_filter_kernel, or nms_filter_ml_kernel with a.multi) unless the workspace is
// `prefiltered` (the fused Detect filter filled it).  Defined in nms.hip.
int nms_launch_filter(const NmsArgs& a, bool prefiltered, hipStream_t st);

// Bitonic sort of P2 (a power of two) keys by the THREADS threads of a workgroup, one compare-exchange pair per thread per pass; every
// thread of the workgroup calls it.  Instantiated per address space (LDS / global) on purpose: a pointer select between the two makes
// the compiler fall back to generic (flat) accesses, which were ~10x slower per pass.
template <int THREADS, typename K>
__device__ __forceinline__ void nms_bitonic_sort(K* keys, int P2, int tid) {
  for (int k = 2; k <= P2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P2 >> 1); t += THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // element with bit j clear
        const int ixj = i | j;
        const u64 x = keys[i], y = keys[ixj];
        const bool up = (i & k) == 0;
        if ((x > y) == up) {
          keys[i] = y;
          keys[ixj] = x;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace dy
