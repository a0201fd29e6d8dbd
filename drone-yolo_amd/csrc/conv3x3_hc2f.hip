// The tail of a hidden-64 C2f block at stride 8 in one kernel (16-bit storage): the last Bottleneck's second 3x3 convolution and the
// block's closing 1x1,
//
//   y_last = SiLU(conv3x3 64->64 (t) + b3) [+ y_prev]            (Bottleneck.forward block.py:348-350, cv2 of the last m)
//   out    = SiLU(conv1x1 (2 + n) * 64 -> 128 (y0 | y1 | .. | y_last) + b1)      (C2f.forward block.py:237-242, self.cv2)
//
// Why: layer by layer the 3x3 (conv3x3_hreg / conv3x3_halo) leaves HBM idle, the 1x1 (conv1x1_stream, at the copy rate) leaves the matrix
// pipe idle, and y_last — a quarter / a third of the concat buffer — is written and read back (0.42 GB per block at B = 256, 80 x 80).
// Here y_last never leaves the CU and the two limits overlap.
//
// The 3x3 part is the family's stride-1 form (hreg_core.h: HrS1).  The tail follows conv3x3_hhead: the tile's 3x3 output is rounded to the storage type exactly where the
// layer-by-layer path rounds it and laid down in the `mid` image ([chunk 2][row 8][pixel 16] x 64 B, the halo's part swizzle); the 1x1
// then runs on MFMAs with K over the NOP leading 64-channel groups of the concat buffer and `mid` (C2f.cv2's input order: buffer
// channels first, the fused 3x3's output last).
//
// A tile is 2 (+ 1 with RES) + NOP items through one two-stage ring of 16 KB stages: the two halo chunks, then the CENTRE pixels of each operand
// group (128 pixels x 64 channels = 16 KB, DMA'd straight into mid's format).  Every item issues the next item's DMA first and ends
// with the full drain + barrier of the family (hreg_core.h: the drain rule).  The 1x1's weight fragments are
// not resident (48 / 64 KB): a wave streams the 1 KB blocks of its two 16-cout fragments per item from L2, requested at the end of the
// item before, in front of the drain that covers them.  With RES (shortcut) y_prev's image gets an item of its own behind the halo chunks:
// it has landed when the item starts, and the 3x3's epilogue runs there and reads the residual from LDS in accumulator layout (no per-lane
// global reads).  The 1x1 sums its K in ascending order from zero and adds the bias last, as conv1x1_stream does, and the 3x3 sums as
// conv3x3_hreg / conv3x3_halo do: the launch computes what its two launches compute, bit for bit.
//
// A wave takes all 32 of its output channels at once: 64 accumulator registers beside the 72 weight registers, two workgroups per CU.
// (Two passes of 16 channels at three workgroups per CU need every operand of the tile resident at once, which costs the ring its
// overlap with the next tile; not built.)
#include "common_hip.h"
#include "hreg_core.h"

namespace DY_NS {

struct Hc2fArgs {
  const void* t;      // 3x3 input, NHWC (N, H, W, 64), pitch ldt
  const void* w3;     // 3x3 64->64, DY_WLAYOUT_HALO3X3 (NF = 4)
  const float* b3;    // 64
  const void* buf;    // concat buffer head y0 | .. , NHWC (N, H, W, NOP * 64), pitch ldb
  const void* w1;     // 1x1 (NOP + 1) * 64 -> 128, DY_WLAYOUT_FRAG1X1 (NF = 8)
  const float* b1;    // 128
  void* y;            // NHWC (N, H, W, 128), pitch ldy
  int N, H, W, ldt, ldb, ldy;
  unsigned t_bytes, b_bytes, y_bytes;
  int tilesX, tilesY, nSpatial;
};

constexpr int kHcTH = HrS1::TH, kHcTW = HrS1::TW;
constexpr int kHcStage = HrS1::kStage;
constexpr int kHcMid = 2 * kHcTH * kHcTW * 64;  // 16 KB: [chunk][row][pixel] x 64 B, the format of an operand stage too

template <typename T, int NOP, bool RES>
__global__ __launch_bounds__(256, 2) void conv3x3_hc2f_kernel(const Hc2fArgs p) {
  constexpr int EPC = Elem<T>::EPC;  // 8
  constexpr int NCH = 2, NRI = RES ? 1 : 0, NIT = NCH + NRI + NOP;  // items per tile: halo chunks, (residual image), operand groups
  constexpr int NF1 = 8;  // 16-cout fragments per k-group of the 1x1 image (cout 128)
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * kHcStage + kHcMid];
  unsigned char* const mid = smem + 2 * kHcStage;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane >> 4, lr = lane & 15;

  const int G = (int)gridDim.x;
  const int sb = hr_block(G, 1).sb;
  const int myTiles = hr_my_tiles(p.nSpatial, sb, G);
  if (myTiles <= 0) return;
  const int nItems = myTiles * NIT;

  // ---- register-resident weights: the wave's 16-cout fragment of the 3x3 ----
  u32x4 wreg[NCH][9];
  hr_load_wreg<NCH>(wreg, reinterpret_cast<const u32x4*>(p.w3), wave, lane);
  const f32x4 bias3 = *reinterpret_cast<const f32x4*>(p.b3 + wave * 16 + lq * 4);
  f32x4 bias1[2];  // the wave's output channels: fragments 2 wave, 2 wave + 1 (32 wave .. + 31)
#pragma unroll
  for (int f = 0; f < 2; ++f) bias1[f] = *reinterpret_cast<const f32x4*>(p.b1 + (wave * 2 + f) * 16 + lq * 4);

  // ---- 1x1 weights: streamed per item.  k-group g (32 channels), fragment j: the 1 KB block (g * 8 + j) of the image ----
  constexpr unsigned kOob = kHrOob;
  const __amdgpu_buffer_rsrc_t w1rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w1), 0, (NOP + 1) * 2 * NF1 * 1024, 0x00020000);
  u32x4 w1a[2][2], w1m[2][2];  // [k-group of the 64-channel group][fragment]: the item's operand group / `mid`
  auto load_w1 = [&](u32x4 (&w)[2][2], int group) {
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
      for (int f = 0; f < 2; ++f) w[c2][f] = __builtin_amdgcn_raw_buffer_load_b128(w1rs, lane * 16, ((group * 2 + c2) * NF1 + wave * 2 + f) * 1024, 0);
  };
  // Items of a tile behind the halo chunks.  The operand groups run in ASCENDING K order, `mid` last, from a zero accumulator with the bias
  // added in the epilogue: the summation of conv1x1_stream, so the result is the two-launch path's bit for bit.  With RES the 3x3's
  // epilogue needs y_prev (the last group) in LDS before `mid` can be written, and its place in the K order is late: its image is
  // fetched twice — an item of its own (kind NCH: residual only, no MFMAs; the second fetch hits L2) and the group's regular item.
  auto group_of_kind = [](int kind) constexpr { return (RES && kind == NCH) ? NOP - 1 : kind - NCH - NRI; };

  // ---- loaders ----
  constexpr int NDMA = HrS1::NDMA;  // every wave issues 4 wave-instructions per item (1 KB each: w, w + 4, w + 8, w + 12), halo and operand alike
  const unsigned pre = (unsigned)((p.W + 1) * p.ldt) * 2u;
  const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.t)) - pre, 0, p.t_bytes + pre, 0x00020000);
  const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.buf), 0, p.b_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.y_bytes, 0x00020000);
  unsigned rel[NDMA];   // halo: ((hy W + hx) ldt + part') * 2
  unsigned orel[NDMA];  // operand: block i = k * 4 + wave is (chunk i >> 3, row i & 7): ((row W + pixel) ldb + chunk * 32 + part' * 8) * 2
  hr_halo_rel<HrS1>(rel, wave, lane, p.W, p.ldt, 2u, 2u * EPC);
#pragma unroll
  for (int k = 0; k < NDMA; ++k) {
    const int i = k * 4 + wave, px = lane >> 2;
    orel[k] = (unsigned)(((i & 7) * p.W + px) * p.ldb + (i >> 3) * 4 * EPC + ((lane & 3) ^ ((px >> 1) & 3)) * EPC) * 2u;
  }
  unsigned voff[NDMA];
  unsigned l_base_t = 0, l_base_b = 0;
  int l_y0 = 0, l_x0 = 0;
  int l_tile = sb, l_item = 0;
  auto setup_tile = [&](int tile) {
    const HrTile t = hr_tile(tile, p.tilesX, p.tilesY);
    const int y0 = t.ty * kHcTH, x0 = t.tx * kHcTW;
    l_y0 = y0, l_x0 = x0;
    l_base_t = (unsigned)(((t.n * p.H + y0) * p.W + x0) * p.ldt) * 2u;
    l_base_b = (unsigned)(((t.n * p.H + y0) * p.W + x0) * p.ldb) * 2u;
    if (hr_interior<HrS1>(y0, x0, p.H, p.W)) {
#pragma unroll
      for (int k = 0; k < NDMA; ++k) voff[k] = rel[k];
    } else {  // the mask again, on border tiles only
#pragma unroll
      for (int k = 0; k < NDMA; ++k) voff[k] = hr_halo_inside<HrS1>(k, wave, lane, y0, x0, p.H, p.W) ? rel[k] : kOob;
    }
  };
  // DMA of the loader's item into `stage`, then advance the loader.  `kind` is the item's place in its tile (a compile-time constant at
  // every call: the loader runs exactly one item ahead of the compute).
  auto issue_dma = [&](int stage, int kind) {
    if (l_item >= nItems) return;  // (wave-uniform)
    unsigned char* sa = smem + stage * kHcStage;
    if (kind < NCH) {
      hr_issue<NDMA>(trs, sa, wave, voff, l_base_t + (unsigned)kind * (4u * EPC * (unsigned)sizeof(T)));
    } else {
      const unsigned soff = l_base_b + (unsigned)group_of_kind(kind) * (64u * (unsigned)sizeof(T));
      const bool whole = l_y0 + kHcTH <= p.H && l_x0 + kHcTW <= p.W;  // wave-uniform
#pragma unroll
      for (int k = 0; k < NDMA; ++k) {
        unsigned vo = orel[k];
        if (!whole) vo = (l_y0 + ((k * 4 + wave) & 7) < p.H && l_x0 + (lane >> 2) < p.W) ? vo : kOob;
        hr_issue1(brs, sa, k, wave, vo, soff);
      }
    }
    ++l_item;
    if (kind == NIT - 1) {
      l_tile += G;
      if (l_item < nItems) setup_tile(l_tile);
    }
  };

  int lane_base[3];
  HrS1::lane_base(lane_base, lr, lq);

  f32x4 acc[kHcTH];       // 3x3: 16 couts x (8 rows x 16 pixels)
  f32x4 acc1[2][kHcTH];   // 1x1: 2 x 16 couts x (8 rows x 16 pixels)

  // 1x1 over one 64-channel operand image (a ring stage or `mid`): one fragment read feeds both of the wave's cout fragments
  auto gemm1 = [&](const unsigned char* img, const u32x4 (&w)[2][2]) {
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
      for (int o = 0; o < kHcTH; ++o) {
        const u32x4 b = *reinterpret_cast<const u32x4*>(img + lane_base[0] + c2 * (kHcTH * kHcTW * 64) + o * (kHcTW * 64));
#pragma unroll
        for (int f = 0; f < 2; ++f) acc1[f][o] = Elem<T>::mma(w[c2][f], b, acc1[f][o]);
        if ((o & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // (at most four fragment reads ahead: hoisted all 16, the reads cost 64 registers and the kernel spilled)
      }
  };

  const int mid_w = hr_mid_offset(wave, lr, lq, kHcTH * kHcTW * 64);  // + o * 1024
  // the 3x3's epilogue: SiLU (+ y_prev from its operand image `resimg`), ONE rounding to the storage type, into `mid`
  auto tail_mid = [&](const unsigned char* resimg) { hr_tail_mid<T, kHcTH, RES>(acc, mid + mid_w, resimg + mid_w); };

  // output: quarter lq stores channels f * 16 + 8 (lq >> 1) .. + 7 of the wave's 32, row o + (lq & 1), column lr
  unsigned lane_out[kHcTH / 2];
  hr_lane_out<kHcTH>(lane_out, lr, lq, p.W, p.ldy, wave * 32 + (lq >> 1) * 8, (unsigned)sizeof(T));
  auto epilogue = [&](int tile) {
    const HrTile t = hr_tile(tile, p.tilesX, p.tilesY);
    const int y0 = t.ty * kHcTH, x0 = t.tx * kHcTW;
    const unsigned out_base = (unsigned)(((t.n * p.H + y0) * p.W + x0) * p.ldy) * (unsigned)sizeof(T);  // scalar
    hr_out_1x1<T, kHcTH>(acc1, bias1, lane_out, yrs, out_base, y0, x0, p.H, p.W, lr, lq);
  };

  // ---- item pipeline: two stages, the next item's DMA in flight during this item's MFMAs, one drain + barrier per item ----
  setup_tile(l_tile);
  issue_dma(0, 0);
  __builtin_amdgcn_s_waitcnt(kHrVmcnt0);
  __syncthreads();
  int c_tile = sb;
  int stage = 0;  // (where NIT is odd an item kind changes its stage from tile to tile)
  for (int it = 0; it < nItems; it += NIT) {
#pragma unroll
    for (int kind = 0; kind < NIT; ++kind) {
      issue_dma(stage ^ 1, (kind + 1) % NIT);  // the other stage was last read one item ago: every wave has passed that item's barrier
      const unsigned char* sa = smem + stage * kHcStage;
      if (kind < NCH) {
        if (kind == 0) {
#pragma unroll
          for (int o = 0; o < kHcTH; ++o) acc[o] = bias3;
        }
        hr_rows_s1<T, NCH>(acc, wreg, sa, lane_base, kind);
        if (kind == NCH - 1) load_w1(w1a, 0);  // (for the tile's first operand item: covered by this item's drain — and by the residual item's)
      } else if (RES && kind == NCH) {
        tail_mid(sa);  // this item's image is y_prev.  `mid` is published by this item's barrier and read in the tile's last item.
      } else {
        const int j = kind - NCH - NRI;
        if (j == 0) {
          if constexpr (!RES) tail_mid(sa);  // published by this item's barrier, read in the tile's last item (NOP >= 2)
#pragma unroll
          for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int o = 0; o < kHcTH; ++o) acc1[f][o] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        gemm1(sa, w1a);
        if (j < NOP - 1) {
          load_w1(w1a, j + 1);
          if (j == NOP - 2) load_w1(w1m, NOP);
        } else {
          gemm1(mid, w1m);
          hr_settle_mfma();
          epilogue(c_tile);
          c_tile += G;
        }
      }
      __builtin_amdgcn_s_waitcnt(kHrVmcnt0);  // (the builtin: the compiler then knows that the streamed weight registers are valid)
      __syncthreads();  // next item's image complete and visible; `mid` written; the output stores retired
      stage ^= 1;
    }
  }
}

template <typename T>
static int launch_hc2f(const Hc2fArgs& a, int nop, bool res, hipStream_t st) {
  const int grid = hr_grid(2, a.nSpatial, 1);  // two 256-thread workgroups per CU (136 weight + accumulator registers per lane)
  const dim3 g((unsigned)grid), b(256);
  if (nop == 2) {
    if (res) hipLaunchKernelGGL((conv3x3_hc2f_kernel<T, 2, true>), g, b, 0, st, a);
    else hipLaunchKernelGGL((conv3x3_hc2f_kernel<T, 2, false>), g, b, 0, st, a);
  } else {
    if (res) hipLaunchKernelGGL((conv3x3_hc2f_kernel<T, 3, true>), g, b, 0, st, a);
    else hipLaunchKernelGGL((conv3x3_hc2f_kernel<T, 3, false>), g, b, 0, st, a);
  }
  return check_launch("conv3x3_hc2f_kernel");
}

}  // namespace DY_NS

using namespace DY_NS;

#ifndef DYOLO_L2E_BUILD
extern "C" int32_t dy_c2f_tail_fused_supported(int32_t hidden, int32_t cout, int32_t n_bottlenecks, int32_t ksize1, int32_t ksize2, int32_t groups, int32_t dtype) {
  if (!(dtype == DY_BF16 || dtype == DY_F16)) return 0;
  return hidden == 64 && cout == 128 && (n_bottlenecks == 1 || n_bottlenecks == 2) && ksize1 == 3 && ksize2 == 3 && groups == 1;
}

namespace dy_l2e {
int32_t c2f_tail_entry(const dy_c2f_tail_desc* d, dy_stream_t stream);
}
namespace dy {
int32_t c2f_tail_entry(const dy_c2f_tail_desc* d, dy_stream_t stream);
}
extern "C" int32_t dy_c2f_tail_fused(const dy_c2f_tail_desc* d, dy_stream_t stream) {
  return (d != nullptr && d->act_l2e) ? dy_l2e::c2f_tail_entry(d, stream) : dy::c2f_tail_entry(d, stream);
}
#endif

namespace DY_NS {
int32_t c2f_tail_entry(const dy_c2f_tail_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->t && d->buf && d->y && d->w3 && d->b3 && d->w1 && d->b1, DY_ERR_INVALID_ARG, "dy_c2f_tail_fused: null pointer");
  DY_REQUIRE(dy_c2f_tail_fused_supported(d->hidden, d->cout, d->n_bottlenecks, 3, 3, 1, d->dtype), DY_ERR_UNSUPPORTED,
             "dy_c2f_tail_fused: built for hidden 64, cout 128, 1 or 2 Bottlenecks, 16-bit storage (got %d / %d / %d dtype %d): run the two dy_conv2d_nhwc calls", d->hidden,
             d->cout, d->n_bottlenecks, d->dtype);
  const int nop = 1 + d->n_bottlenecks;
  DY_REQUIRE(d->batch > 0 && d->h > 0 && d->w > 0 && d->ld_t >= d->hidden && d->ld_buf >= nop * d->hidden && d->ld_y >= d->cout, DY_ERR_INVALID_ARG,
             "dy_c2f_tail_fused: bad dims / pitches");
  DY_REQUIRE(d->ld_t % 8 == 0 && d->ld_buf % 8 == 0 && d->ld_y % 8 == 0 && aligned16(d->t) && aligned16(d->buf) && aligned16(d->y) && aligned16(d->w3) && aligned16(d->w1) &&
                 aligned16(d->b3) && aligned16(d->b1),
             DY_ERR_INVALID_ARG, "dy_c2f_tail_fused: views must be whole 16-byte chunks");
  const long long px = (long long)d->batch * d->h * d->w;
  DY_REQUIRE(px * d->ld_t * 2 < (1ll << 31) && px * d->ld_buf * 2 < (1ll << 31) && px * d->ld_y * 2 < (1ll << 32) - 64, DY_ERR_UNSUPPORTED,
             "dy_c2f_tail_fused: a view exceeds 2 GiB (32-bit offsets)");
  Hc2fArgs a{};
  a.t = d->t, a.w3 = d->w3, a.b3 = d->b3, a.buf = d->buf, a.w1 = d->w1, a.b1 = d->b1, a.y = d->y;
  a.N = d->batch, a.H = d->h, a.W = d->w, a.ldt = d->ld_t, a.ldb = d->ld_buf, a.ldy = d->ld_y;
  a.t_bytes = (unsigned)(px * d->ld_t * 2), a.b_bytes = (unsigned)(px * d->ld_buf * 2), a.y_bytes = (unsigned)(px * d->ld_y * 2);
  a.tilesX = (d->w + kHcTW - 1) / kHcTW, a.tilesY = (d->h + kHcTH - 1) / kHcTH;
  a.nSpatial = d->batch * a.tilesX * a.tilesY;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool res = d->shortcut != 0;
  return d->dtype == DY_BF16 ? launch_hc2f<bf16_t>(a, nop, res, st) : launch_hc2f<f16_t>(a, nop, res, st);
}
}  // namespace DY_NS
