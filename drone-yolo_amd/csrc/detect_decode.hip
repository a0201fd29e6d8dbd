// Detect decode of all levels in one launch, fp32 throughout, with the NMS candidate filter optionally fused in.  The decode of a
// row and the filter's append are detect_row.h's.  Reference: nn/modules/head.py:100-131 (_inference).
//
// A single-wave workgroup owns 64 consecutive anchors of one (image, level).  Their head rows
// (4*reg_max + nc logits each, pitch ld) are one contiguous span of the NHWC head buffer, so it is
// copied to LDS with lane-linear 16-byte loads (every fetched byte is used once; a lane-per-row
// float4 read pattern fetched ~4x the bytes) and each lane then reads its own row from LDS.
// Writes: out[b][ch][a] — consecutive lanes are consecutive anchors, every channel row a coalesced store.
#include "detect_row.h"

namespace dy {

constexpr int kDecTile = 64;  // one wave per tile: 64 rows x pitch floats of LDS (19 KB at pitch 76), 8 tiles resident per CU

struct DecodeArgs {
  const float* level[DY_MAX_LEVELS];
  int h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS], a0[DY_MAX_LEVELS + 1], t0[DY_MAX_LEVELS + 1];
  float stride[DY_MAX_LEVELS];
  int n_levels, batch, nc, A, tilesPerImg;
  float* out;
  FilterSink f;  // fused NMS filter (optional)
};

template <int REG_MAX>
__global__ __launch_bounds__(64) void detect_decode_kernel(const DecodeArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  float* rows = reinterpret_cast<float*>(dyn_smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x / p.tilesPerImg;
  const int tr = blockIdx.x - b * p.tilesPerImg;
  int l = 0;
#pragma unroll
  for (int i = 1; i < DY_MAX_LEVELS; ++i)
    if (i < p.n_levels && tr >= p.t0[i]) l = i;
  const int hw = p.h[l] * p.w[l];
  const int al0 = (tr - p.t0[l]) * kDecTile;           // first anchor of the tile inside the level
  const int na = (hw - al0) < kDecTile ? (hw - al0) : kDecTile;
  const int ld = p.ld[l];
  const float* src = p.level[l] + ((size_t)b * hw + al0) * (size_t)ld;
  const int n4 = na * ld / 4;  // ld % 4 == 0
  for (int i = tid; i < n4; i += kDecTile) reinterpret_cast<f32x4*>(rows)[i] = reinterpret_cast<const f32x4*>(src)[i];
  __syncthreads();  // single wave: orders the LDS writes before the row reads

  const bool valid = tid < na;
  const int al = al0 + tid;
  const int a = p.a0[l] + al;
  RowBest rb{0.f, 0};
  if (valid) {
    const int gy = al / p.w[l], gx = al - gy * p.w[l];
    rb = detect_decode_row<REG_MAX>(rows + tid * ld, 4 * REG_MAX, gx, gy, p.stride[l], p.out + (size_t)b * (size_t)(4 + p.nc) * p.A, a, p.A, p.nc);
  }
  if (p.f.keys != nullptr) filter_append(p.f, lane, valid, rb, b, a, p.A);  // one image per workgroup, so one append per wave
}

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_detect_decode(const dy_decode_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->out, DY_ERR_INVALID_ARG, "dy_detect_decode: null descriptor/out");
  DY_REQUIRE(d->n_levels >= 1 && d->n_levels <= DY_MAX_LEVELS && d->batch > 0 && d->nc > 0, DY_ERR_INVALID_ARG,
             "dy_detect_decode: bad n_levels/batch/nc");
  DY_REQUIRE(d->reg_max == 16, DY_ERR_UNSUPPORTED, "dy_detect_decode: reg_max %d not built (only 16)", d->reg_max);
  DecodeArgs a{};
  int A = 0, T = 0, ldmax = 0;
  for (int i = 0; i < d->n_levels; ++i) {
    DY_REQUIRE(d->level[i] && d->h[i] > 0 && d->w[i] > 0, DY_ERR_INVALID_ARG, "dy_detect_decode: level %d null/empty", i);
    DY_REQUIRE(d->ld[i] >= 4 * d->reg_max + d->nc && d->ld[i] % 4 == 0 && aligned16(d->level[i]), DY_ERR_INVALID_ARG,
               "dy_detect_decode: level %d pitch %d must be >= %d, a multiple of 4 floats, base 16B aligned", i, d->ld[i],
               4 * d->reg_max + d->nc);
    a.level[i] = d->level[i];
    a.h[i] = d->h[i];
    a.w[i] = d->w[i];
    a.ld[i] = d->ld[i];
    a.stride[i] = d->stride[i];
    a.a0[i] = A;
    a.t0[i] = T;
    A += d->h[i] * d->w[i];
    T += (d->h[i] * d->w[i] + kDecTile - 1) / kDecTile;
    if (d->ld[i] > ldmax) ldmax = d->ld[i];
  }
  a.a0[d->n_levels] = A;
  a.t0[d->n_levels] = T;
  a.n_levels = d->n_levels;
  a.batch = d->batch;
  a.nc = d->nc;
  a.A = A;
  a.tilesPerImg = T;
  a.out = d->out;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->nms_workspace) {
    const int rc = filter_sink_from_workspace("dy_detect_decode", d->nms_workspace, d->nms_workspace_bytes, d->batch, A, d->nc, d->conf_thres, d->classes_mask, &a.f);
    if (rc != DY_OK) return rc;
    zero_async(a.f.counts, (size_t)d->batch * 4, st);
  }
  const size_t smem = (size_t)kDecTile * ldmax * 4;
  DY_REQUIRE(smem <= 160 * 1024, DY_ERR_UNSUPPORTED, "dy_detect_decode: head pitch %d too large for the LDS tile", ldmax);
  static const hipError_t once = hipFuncSetAttribute((const void*)detect_decode_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)once;
  hipLaunchKernelGGL((detect_decode_kernel<16>), dim3((unsigned)(d->batch * T)), dim3(kDecTile), smem, st, a);
  return check_launch("detect_decode_kernel");
}
