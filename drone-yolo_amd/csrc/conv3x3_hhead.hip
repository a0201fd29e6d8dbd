// One Detect branch from its second 3x3 convolution to the decoded output, in one kernel (16-bit storage):
//
//   box branch (KIND 1):  Conv 3x3 64->64 + SiLU  ->  Conv2d 1x1 64->64 (+bias)  ->  DFL softmax expectation per side
//                         ->  dist2bbox with the anchor grid, x stride  ->  rows 0..3 of pred (N, 4 + nc, A)
//   class branch (KIND 2): Conv 3x3 64->64 + SiLU  ->  Conv2d 1x1 64->nc (+bias)  ->  sigmoid  ->  rows 4.. of pred,
//                         best class / score per anchor  ->  NMS candidate list (conf filter, optional class mask)
//
// Reference: Detect.forward head.py:64-70 (cv2[i][1], cv2[i][2], cv3[i][1], cv3[i][2] of the legacy v8 head, head.py:43-57),
// Detect._inference head.py:100-131, DFL block.py:58-76, make_anchors / dist2bbox tal.py:333-357, the candidate filter of
// non_max_suppression ops.py:250,290-295.
//
// Why: layer by layer the trunk outputs (34,000 anchors x 2 branches x 64 channels) are written by the 3x3 kernels and read
// back by the fused tail (detect_head.hip): 256 B per anchor each way, 4.5 GB per pass at B = 256 — the tail runs at the HBM
// rate and cannot get faster on its own.  Here the 3x3 output tile never leaves the CU: it is rounded to the storage type
// exactly where the layer-by-layer path rounds it, laid down in LDS in the halo image's format, and consumed by the 1x1 MFMAs.
//
// The 3x3 part is the family's stride-1 form (hreg_core.h: HrS1, two stages, three 256-thread workgroups per CU).  After the tile's two chunks:
//   1. every wave SiLUs its 16 couts x 128 pixels and writes them (8 bytes per lane) into the `mid` image
//      [chunk 2][row 8][pixel 16] x 64 B with the halo's part swizzle; barrier;
//   2. 1x1: the wave's A fragment(s) sit in 8 registers; B fragments are conflict-free ds_read_b128 of `mid`.
//      Box: wave w computes side w (16 bins) for all 8 rows: 16 MFMAs.  Class: the waves split the rows (2 each): 4 MFMAs;
//   3. box: a lane holds 4 of a side's 16 bins of one pixel; the softmax expectation is reduced over the four lane quarters with
//      two xor-shuffles; the four sides meet through 2 KB of LDS and 256 threads write (cx, w) / (cy, h) of the 128 pixels;
//      class: sigmoid per class, first arg-max over the quarters by shuffles (lowest class wins ties, as cls.max(1)), ballot +
//      one atomicAdd per wave to append the candidates (the key of detect_row.h's wave_append, stored by hand a tile later).
#include "detect_row.h"
#include "hreg_core.h"

namespace DY_NS {


struct HheadArgs {
  const void* x;       // trunk input, NHWC (N, H, W, 64), pitch ldx
  const void* w3;      // 3x3 64->64, DY_WLAYOUT_HALO3X3 (NF = 4)
  const float* b3;     // 64
  const void* w1;      // 1x1, DY_WLAYOUT_FRAG1X1: box cout 64 (4 fragments per k-group), class cout nc <= 16 (1 fragment)
  const float* b1;     // 64 / 16
  float* out;          // pred (N, 4 + nc, A) fp32
  int N, H, W, ldx, A, a0, nc;
  unsigned x_bytes;
  float stride;
  int tilesX, tilesY, nSpatial;
  FilterSink f;  // NMS candidate filter of the class branch (optional)
};

constexpr int kHhTH = HrS1::TH, kHhTW = HrS1::TW;
constexpr int kHhStage = HrS1::kStage, kHhStages = 2;
constexpr int kHhMid = 2 * kHhTH * kHhTW * 64;  // 16 KB: the tile's 3x3 output, [chunk][row][pixel] x 64 B

// Exchange between the four 16-lane quarters of a wave without touching LDS (v_permlane16_swap / v_permlane32_swap, gfx950):
// quarter_pair(v): every lane gets (its own quarter pair's two values) -> combine with op: rows {0,1} and {2,3}; half_pair: {0,1} with {2,3}.
__device__ __forceinline__ void quarter_views(float v, float& a, float& b) {  // a = rows (0,0,2,2), b = rows (1,1,3,3) of v
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
__device__ __forceinline__ void half_views(float v, float& a, float& b) {  // a = rows (0,1,0,1), b = rows (2,3,2,3) of v
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
__device__ __forceinline__ float wave_quarters_max(float v) {
  float a, b;
  quarter_views(v, a, b);
  v = fmaxf(a, b);
  half_views(v, a, b);
  return fmaxf(a, b);
}
__device__ __forceinline__ float wave_quarters_sum(float v) {
  float a, b;
  quarter_views(v, a, b);
  v = a + b;
  half_views(v, a, b);
  return a + b;
}

template <typename T, int KIND>
__global__ __launch_bounds__(256, 3) void conv3x3_hhead_kernel(const HheadArgs p) {
  constexpr int EPC = Elem<T>::EPC;  // 8
  constexpr int NCH = 2;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[kHhStages * kHhStage + kHhMid + 4 * kHhTH * kHhTW * 4];
  unsigned char* const mid = smem + kHhStages * kHhStage;
  float* const dsm = reinterpret_cast<float*>(mid + kHhMid);  // [side 4][pixel 128]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave: a scalar, it enters scalar store offsets)
  const int lq = lane >> 4, lr = lane & 15;

  const int G = (int)gridDim.x;
  const int sb = hr_block(G, 1).sb;
  const int myTiles = hr_my_tiles(p.nSpatial, sb, G);
  if (myTiles <= 0) return;
  const int nItems = myTiles * NCH;

  // ---- register-resident weights: the wave's 16-cout fragment of the 3x3 ----
  u32x4 wreg[NCH][9];
  hr_load_wreg<NCH>(wreg, reinterpret_cast<const u32x4*>(p.w3), wave, lane);
  const f32x4 bias3 = *reinterpret_cast<const f32x4*>(p.b3 + wave * 16 + lq * 4);
  // The 1x1 fragments (2 x 16 B per lane) and its bias are re-read per tile (L2 / L1 hits): 12 registers the 3x3 loop needs more.
  // r06: they are requested at the END of the tile's last item (load_w1, in front of tail_mid), so that the item's closing drain covers
  // them.  Requested inside tail_out they were younger than the next item's halo DMA, and vmcnt retires in order: their first use made
  // every wave wait for the DMA it had just issued, once per tile.
  constexpr unsigned kOob = kHrOob;
  const __amdgpu_buffer_rsrc_t w1rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w1), 0, NCH * (KIND == 1 ? 4 : 1) * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t b1rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.b1), 0, (KIND == 1 ? 64 : 16) * 4, 0x00020000);
  u32x4 w1reg[NCH];
  f32x4 bias1;
  auto load_w1 = [&]() {
#pragma unroll
    for (int c = 0; c < NCH; ++c) w1reg[c] = __builtin_amdgcn_raw_buffer_load_b128(w1rs, lane * 16, (c * (KIND == 1 ? 4 : 1) + (KIND == 1 ? wave : 0)) * 1024, 0);
    bias1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b1rs, lq * 16, (KIND == 1 ? wave : 0) * 64, 0));
  };

  // ---- halo loader ----
  constexpr int NDMA = HrS1::NDMA;
  const unsigned pre = (unsigned)((p.W + 1) * p.ldx) * 2u;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.x)) - pre, 0, p.x_bytes + pre, 0x00020000);
  unsigned rel[NDMA];
  hr_halo_rel<HrS1>(rel, wave, lane, p.W, p.ldx, 2u, 2u * EPC);
  unsigned voff[NDMA];
  unsigned l_base = 0;
  int l_tile = sb, l_chunk = 0, l_item = 0;
  auto setup_tile = [&](int tile) {
    const HrTile t = hr_tile(tile, p.tilesX, p.tilesY);
    const int y0 = t.ty * kHhTH, x0 = t.tx * kHhTW;
    l_base = (unsigned)(((t.n * p.H + y0) * p.W + x0) * p.ldx) * 2u;
    if (hr_interior<HrS1>(y0, x0, p.H, p.W)) {
#pragma unroll
      for (int k = 0; k < NDMA; ++k) voff[k] = rel[k];
    } else {
      // the slots' halo pixels again, on border tiles only: as a table (or hoisted out of the tile loop, which the empty asm forbids) they cost
      // four registers, and the class branch is then back in scratch (8-12 bytes)
      int ln = lane;
      asm volatile("" : "+v"(ln));
#pragma unroll
      for (int k = 0; k < NDMA; ++k) voff[k] = hr_halo_inside<HrS1>(k, wave, ln, y0, x0, p.H, p.W) ? rel[k] : kOob;
    }
  };
  auto issue_dma = [&](int stage) {
    unsigned char* sa = smem + stage * kHhStage;
    const bool live = l_item < nItems;
    if (live) {
      hr_issue<NDMA>(xrs, sa, wave, voff, l_base + (unsigned)l_chunk * (4u * EPC * (unsigned)sizeof(T)));
      ++l_item;
      if (++l_chunk == NCH) {
        l_chunk = 0;
        l_tile += G;
        if (l_item < nItems) setup_tile(l_tile);
      }
    } else {
#pragma unroll
      for (int k = 0; k < NDMA; ++k) hr_issue1(xrs, sa, k, wave, kOob, 0u);
    }
  };

  int lane_base[3];
  HrS1::lane_base(lane_base, lr, lq);

  f32x4 acc[kHhTH];

  // ---- the tail of one tile ----
  const int mid_w = hr_mid_offset(wave, lr, lq, kHhTH * kHhTW * 64);  // + o * 1024
  const int mid_r = lane_base[0];                                                                                                          // + c2 * 8192 + o * 1024
  // tail, part 1 (end of the tile's last item): SiLU, round to the storage type (where the layer-by-layer path rounds), into `mid`.
  // The item's closing barrier publishes it.
  auto tail_mid = [&]() { hr_tail_mid<T, kHhTH, false>(acc, mid + mid_w, nullptr); };
  // tail, part 2, DEFERRED to the start of the next item (after that item's DMA has been issued, before its MFMAs): the global
  // stores then have a whole item of matrix work behind them before the item's closing s_waitcnt vmcnt(0), instead of being waited
  // for right after they were issued (first version: the fused kernels cost as much as conv + separate tail kernel)
  // class branch: the candidate append of a tile is FINISHED one tile later (r04).  The counter atomic returns the wave's slot range;
  // the first form used it at once — every wave stood still for the round trip (1-2 us of an 11 us tile, in front of the item's MFMAs):
  // the class branch ran 17 % slower than the box branch for 1/6 of its 1x1 work.  Now the atomic is issued at the end of tail_out and
  // its value read at the start of the next one (or after the last tile): it returns under a whole item of matrix work.
  // r06: nothing in tail_out waits for vector memory.  Every store goes through a per-image buffer descriptor (a scalar base from the tile id)
  // with a 32-bit lane offset and a scalar offset; lanes outside the map / beyond nc get an out-of-range offset instead of a branch.  The
  // 64-bit store pointers and the candidate state of the first form (two ballot masks, anchors, image) did not fit the 168 registers
  // beside the 3x3 loop: 124 bytes of scratch per lane in the class branch, and every reload was a vector-memory load queued behind the halo DMA.
  // What waits a tile: the two ballot masks and the tile id (scalars), best score / class per row (4 registers), the counter's return (1).
  struct TileAt { int n, y0, x0; };
  auto tile_at = [&](int tile) {
    const HrTile t = hr_tile(tile, p.tilesX, p.tilesY);
    return TileAt{t.n, t.ty * kHhTH, t.tx * kHhTW};
  };
  const unsigned img_bytes = (unsigned)((4 + p.nc) * p.A) * 4u;
  auto out_rsrc = [&](int n) { return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(p.out) + (size_t)n * img_bytes, 0, (int)img_bytes, 0x00020000); };
  unsigned cm_bits = 0xffffu;  // classes_mask as bits (nc <= 16): no byte load behind the DMA in the filter
  if constexpr (KIND == 2) {
    if (p.f.keys != nullptr && p.f.cmask != nullptr) cm_bits = (unsigned)__ballot(lane < p.nc && p.f.cmask[lane < p.nc ? lane : 0] != 0);
  }
  int pv_tile = 0, pv_base = 0;
  unsigned long long pv_mk0 = 0ull, pv_mk1 = 0ull;
  float pv_best[2] = {0.f, 0.f};
  int pv_bj[2] = {0, 0};
  auto flush_keys = [&]() {
    if ((pv_mk0 | pv_mk1) != 0ull) {
      const TileAt t = tile_at(pv_tile);
      const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(p.f.keys + (size_t)t.n * p.f.P, 0, p.f.P * 8, 0x00020000);
      const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(p.f.cls + (size_t)t.n * p.A, 0, p.A * 2, 0x00020000);
      const int base = __builtin_amdgcn_readfirstlane(pv_base);
      const int n0 = __popcll(pv_mk0);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const unsigned long long mk = j ? pv_mk1 : pv_mk0;
        const bool hit = (mk >> lane) & 1ull;  // (lanes of quarter 0 only: lane == lr)
        const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
        const int a_row = p.a0 + (t.y0 + wave * 2 + j) * p.W + t.x0;  // scalar: the anchor of the row's first pixel
        const u32x2 key = {(unsigned)(a_row + lr), ~__float_as_uint(pv_best[j])};  // = ~score bits << 32 | anchor
        __builtin_amdgcn_raw_buffer_store_b64(key, krs, hit ? below * 8u : kOob, (base + (j ? n0 : 0)) * 8, 0);
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)pv_bj[j], crs, hit ? (unsigned)lr * 2u : kOob, a_row * 2, 0);
      }
      pv_mk0 = pv_mk1 = 0ull;
    }
  };
  auto tail_out = [&](int tile) {
    if constexpr (KIND == 2) flush_keys();
    const TileAt t = tile_at(tile);
    const __amdgpu_buffer_rsrc_t ors = out_rsrc(t.n);
    if constexpr (KIND == 1) {
      // 1x1: side `wave`, bins lq*4 .. +3 of pixel (o, lr); then DFL = softmax expectation over the side's 16 bins
#pragma unroll
      for (int o = 0; o < kHhTH; ++o) {
        f32x4 lg = bias1;
#pragma unroll
        for (int c2 = 0; c2 < NCH; ++c2)
          lg = Elem<T>::mma(w1reg[c2], *reinterpret_cast<const u32x4*>(mid + mid_r + c2 * (kHhTH * kHhTW * 64) + o * (kHhTW * 64)), lg);
        const float m = wave_quarters_max(fmaxf(fmaxf(lg[0], lg[1]), fmaxf(lg[2], lg[3])));
        float den = 0.f, num = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float ex = __builtin_amdgcn_exp2f((lg[e] - m) * 1.4426950408889634f);
          den += ex;
          num += ex * (float)(lq * 4 + e);
        }
        den = wave_quarters_sum(den);
        num = wave_quarters_sum(num);
        if (lq == 0) dsm[wave * (kHhTH * kHhTW) + o * kHhTW + lr] = num * __builtin_amdgcn_rcpf(den);
      }
      // (a raw barrier: __syncthreads' release fence also drains the vector-memory counter, that is the halo DMA issued a moment ago)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // dist2bbox (tal.py:348-357) x stride: thread -> (pixel, axis); sides: 0 left, 1 top, 2 right, 3 bottom
      const int px = tid & 127, axis = tid >> 7;
      const int o = px >> 4, xi = px & 15;
      const int yy = t.y0 + o, xx = t.x0 + xi;
      const float d_lo = dsm[axis * (kHhTH * kHhTW) + px], d_hi = dsm[(axis + 2) * (kHhTH * kHhTW) + px];
      const float ctr = (float)(axis == 0 ? xx : yy) + 0.5f;
      const float lo = ctr - d_lo, hi = ctr + d_hi;
      const unsigned vo = (yy < p.H && xx < p.W) ? (unsigned)(axis * p.A + o * p.W + xi) * 4u : kOob;
      const int so = (p.a0 + t.y0 * p.W + t.x0) * 4;  // scalar: the tile's first anchor
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((lo + hi) * 0.5f * p.stride), ors, vo, so, 0);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((hi - lo) * p.stride), ors, vo, so + 2 * p.A * 4, 0);
    } else {
      // 1x1 64 -> nc (one 16-cout fragment): the waves split the rows; sigmoid, scores out, first arg-max, candidate filter.
      // The wave's two rows are filtered together: ONE counter atomic (with return: the wave waits for it) per wave and tile
      // instead of one per row - on the P2 level every tile has candidates and the atomics of an image all hit one address.
      bool passv[2];
      const unsigned sc_lane = (unsigned)((4 + lq * 4) * p.A + lr) * 4u;  // row 4 + lq * 4 of pred, column lr
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int o = wave * 2 + j;
        f32x4 lg = bias1;
#pragma unroll
        for (int c2 = 0; c2 < NCH; ++c2)
          lg = Elem<T>::mma(w1reg[c2], *reinterpret_cast<const u32x4*>(mid + mid_r + c2 * (kHhTH * kHhTW * 64) + o * (kHhTW * 64)), lg);
        const bool inside = t.y0 + o < p.H && t.x0 + lr < p.W;
        const int a_row = p.a0 + (t.y0 + o) * p.W + t.x0;  // scalar
        float best = -1.f;
        int bj = 0x7fff;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = lq * 4 + e;
          const float pr = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(lg[e] * -1.4426950408889634f));
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(pr), ors, (inside && c < p.nc) ? sc_lane : kOob, (a_row + e * p.A) * 4, 0);
          if (c < p.nc && pr > best) best = pr, bj = c;  // ascending c: the first maximum stays
        }
#pragma unroll
        for (int sh = 16; sh <= 32; sh <<= 1) {  // the four quarters hold classes 0-3, 4-7, 8-11, 12-15 of this pixel
          const float ob = __shfl_xor(best, sh);
          const int oj = __shfl_xor(bj, sh);
          if (ob > best || (ob == best && oj < bj)) best = ob, bj = oj;
        }
        passv[j] = inside && lq == 0 && best > p.f.conf && ((cm_bits >> (bj & 15)) & 1u) != 0u;
        pv_best[j] = best, pv_bj[j] = bj;
      }
      if (p.f.keys != nullptr) {
        pv_mk0 = __ballot(passv[0]), pv_mk1 = __ballot(passv[1]);
        pv_tile = tile;
        const int total = __popcll(pv_mk0) + __popcll(pv_mk1);
        if (total != 0 && lane == 0) pv_base = atomicAdd(p.f.counts + t.n, total);  // (value used by flush_keys, one tile later)
      }
    }
  };

  // ---- item pipeline: two stages, the next item's DMA in flight during this item's MFMAs, one barrier per item ----
  setup_tile(l_tile);
  issue_dma(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int c_tile = sb, pending = -1;
  for (int it = 0; it < nItems; it += NCH) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      issue_dma((c & 1) ^ 1);  // the other stage was last read one item ago: every wave has passed that item's barrier
      if (c == 0) {
        if (pending >= 0) tail_out(pending);  // the previous tile's 1x1 + decode: `mid` was published by the barrier that ended it
#pragma unroll
        for (int o = 0; o < kHhTH; ++o) acc[o] = bias3;  // (only now: the accumulator registers are free during tail_out)
      }
      hr_rows_s1<T, NCH>(acc, wreg, smem + (c & 1) * kHhStage, lane_base, c);
      if (c == NCH - 1) {
        load_w1();  // (the accumulators' last MFMAs and the SiLU pass cover the round trip; nothing of the 3x3 loop is live beside them but acc)
        tail_mid();
        pending = c_tile;
        c_tile += G;
      }
      __builtin_amdgcn_s_waitcnt(kHrVmcnt0);  // (the builtin, not an asm: the compiler then knows that load_w1's registers and the counter's return are valid)
      __syncthreads();  // next item's halo complete and visible; `mid` written (last chunk) / `dsm` free again; the 1x1 operands landed
    }
  }
  if (pending >= 0) tail_out(pending);
  if constexpr (KIND == 2) flush_keys();  // (the only place where the counter's return is waited for: once per workgroup)
}

template <typename T>
static int launch_hhead(const HheadArgs& a, int kind, hipStream_t st) {
  const int grid = hr_grid(3, a.nSpatial, 1);
  if (kind == 1)
    hipLaunchKernelGGL((conv3x3_hhead_kernel<T, 1>), dim3((unsigned)grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv3x3_hhead_kernel<T, 2>), dim3((unsigned)grid), dim3(256), 0, st, a);
  return check_launch("conv3x3_hhead_kernel");
}

}  // namespace DY_NS

using namespace DY_NS;

#ifndef DYOLO_L2E_BUILD
extern "C" int32_t dy_detect_branch_fused_supported(int32_t c_in, int32_t c_mid, int32_t c_out, int32_t kind, int32_t nc, int32_t reg_max, int32_t dtype) {
  if (!(dtype == DY_BF16 || dtype == DY_F16) || reg_max != 16 || c_in != 64 || c_mid != 64) return 0;
  if (kind == 1) return c_out == 64;
  if (kind == 2) return c_out == nc && nc >= 1 && nc <= 16;
  return 0;
}

namespace dy_l2e {
int32_t branch_entry(const dy_branch_desc* d, dy_stream_t stream);
}
namespace dy {
int32_t branch_entry(const dy_branch_desc* d, dy_stream_t stream);
}
extern "C" int32_t dy_detect_branch_fused(const dy_branch_desc* d, dy_stream_t stream) {
  return (d != nullptr && d->act_l2e) ? dy_l2e::branch_entry(d, stream) : dy::branch_entry(d, stream);
}

extern "C" int32_t dy_nms_reset_counts(void* nms_workspace, int32_t batch, dy_stream_t stream) {
  DY_REQUIRE(nms_workspace && batch > 0, DY_ERR_INVALID_ARG, "dy_nms_reset_counts: bad arguments");
  zero_async(nms_workspace, (size_t)batch * 4, reinterpret_cast<hipStream_t>(stream));
  return check_launch("dy_nms_reset_counts");
}
#endif

namespace DY_NS {
int32_t branch_entry(const dy_branch_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->x && d->w3 && d->b3 && d->w1 && d->b1 && d->out, DY_ERR_INVALID_ARG, "dy_detect_branch_fused: null pointer");
  DY_REQUIRE(dy_detect_branch_fused_supported(d->c_in, d->c_mid, d->kind == 1 ? 4 * d->reg_max : d->nc, d->kind, d->nc, d->reg_max, d->dtype), DY_ERR_UNSUPPORTED,
             "dy_detect_branch_fused: kind %d c_in %d c_mid %d nc %d reg_max %d dtype %d is not built (run dy_conv2d_nhwc + dy_detect_head_decode)", d->kind, d->c_in,
             d->c_mid, d->nc, d->reg_max, d->dtype);
  DY_REQUIRE(d->batch > 0 && d->h > 0 && d->w > 0 && d->ld_x >= d->c_in && (d->ld_x * 2) % 16 == 0 && aligned16(d->x) && aligned16(d->w3) && aligned16(d->w1) &&
                 aligned16(d->b3) && aligned16(d->b1),
             DY_ERR_INVALID_ARG, "dy_detect_branch_fused: views must be whole 16-byte chunks");
  DY_REQUIRE(d->anchors > 0 && d->anchor0 >= 0 && d->anchor0 + d->h * d->w <= d->anchors, DY_ERR_INVALID_ARG, "dy_detect_branch_fused: the level's anchors [%d, %d) exceed A = %d",
             d->anchor0, d->anchor0 + d->h * d->w, d->anchors);
  DY_REQUIRE((long long)d->batch * d->h * d->w * d->ld_x * 2 < (1ll << 31), DY_ERR_UNSUPPORTED, "dy_detect_branch_fused: input view exceeds 2 GiB (32-bit element offsets)");
  DY_REQUIRE((long long)(4 + d->nc) * d->anchors * 4 < (1ll << 31), DY_ERR_UNSUPPORTED, "dy_detect_branch_fused: one image of pred exceeds 2 GiB (32-bit store offsets)");
  HheadArgs a{};
  a.x = d->x, a.w3 = d->w3, a.b3 = d->b3, a.w1 = d->w1, a.b1 = d->b1, a.out = d->out;
  a.N = d->batch, a.H = d->h, a.W = d->w, a.ldx = d->ld_x, a.A = d->anchors, a.a0 = d->anchor0, a.nc = d->nc, a.stride = d->stride;
  a.x_bytes = (unsigned)((long long)d->batch * d->h * d->w * d->ld_x * 2);
  a.tilesX = (d->w + kHhTW - 1) / kHhTW, a.tilesY = (d->h + kHhTH - 1) / kHhTH;
  a.nSpatial = d->batch * a.tilesX * a.tilesY;
  if (d->kind == 2 && d->nms_workspace) {  // (the counts are zeroed once per pass, by dy_nms_reset_counts: every level's class branch appends)
    const int rc = filter_sink_from_workspace("dy_detect_branch_fused", d->nms_workspace, d->nms_workspace_bytes, d->batch, d->anchors, d->nc, d->conf_thres, d->classes_mask, &a.f);
    if (rc != DY_OK) return rc;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return d->dtype == DY_BF16 ? launch_hhead<bf16_t>(a, d->kind, st) : launch_hhead<f16_t>(a, d->kind, st);
}
}  // namespace DY_NS

