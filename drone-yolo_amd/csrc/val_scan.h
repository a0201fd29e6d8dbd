// The second half of the validator's match rule, shared by dy_val_match / dy_val_match_rotated (val_match.hip: box IoU / ProbIoU) and
// dy_val_mask_match (val_mask.hip: mask IoU).  With best(d) / biou(d) of an image's kept rows in LDS (rows in descending confidence, so "e < d" is "ranked higher"):
//     tp[d][i] = biou(d) >= thr[i] and no e < d has best(e) == best(d) and biou(e) >= thr[i]
// Every element of tp / best_iou / best_label of the image is written; rows >= cnt (or without a label) get 0 / 0 / -1.
#pragma once
#include "common_hip.h"

namespace dy {

// best, biou: [cnt] filled by the caller and visible (a barrier behind the writes); prev: [max_det] scratch; thr: [n_iouv], all in LDS.
// Called by every thread of the workgroup (it holds a barrier).  label_base is added to the stored best_label (positions >= 0 only).
__device__ __forceinline__ void val_rank_scan(const int* best, const float* biou, float* prev, const float* thr, int cnt, int max_det, int n_iouv,
                                              uint8_t* tpb, float* best_iou, int* best_label, int label_base, int tid, int nthreads) {
  for (int d = tid; d < cnt; d += nthreads) {
    const int bl = best[d];
    float pm = -1.f;
    if (bl >= 0)
      for (int e = 0; e < d; ++e)
        if (best[e] == bl) pm = fmaxf(pm, biou[e]);
    prev[d] = pm;
  }
  __syncthreads();

  const int total = max_det * n_iouv;
  for (int i = tid; i < total; i += nthreads) {
    const int d = i / n_iouv;
    const float t = thr[i - d * n_iouv];
    bool ok = false;
    if (d < cnt) ok = best[d] >= 0 && biou[d] >= t && !(prev[d] >= t);
    tpb[i] = ok ? 1 : 0;
  }
  for (int d = tid; d < max_det; d += nthreads) {
    const bool has = d < cnt && best[d] >= 0;
    if (best_iou) best_iou[d] = has ? biou[d] : 0.f;
    if (best_label) best_label[d] = has ? best[d] + label_base : -1;
  }
}

}  // namespace dy
