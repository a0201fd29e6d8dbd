// The front of a hidden-64 C2f block at stride 8 in one kernel (16-bit storage): the stride-2 3x3 convolution in front of the block
// and the block's opening 1x1,
//
//   mid = SiLU(conv3x3 s2 64 -> C3 (x) + b3)                                  (Conv / folded RepVGGBlock, conv.py:53-55)
//   out = SiLU(conv1x1 (C3 + NOG * 64) -> 128 (mid | other) + b1)             (C2f.forward block.py:237-242, self.cv1)
//
// form A (C3 = 128, NOG = 0): yaml layers 3 -> 4;  form B (C3 = 64, NOG = 2): layers 19 -> Concat 20 -> 21, `other` is the second Concat
// source (128 channels, a view with its own pitch).
//
// Why: the 3x3's output has one consumer, the 1x1, and layer by layer it is written to HBM and read straight back by a launch that runs
// at the copy rate (conv1x1_stream) while the matrix pipe idles.  Here `mid` never leaves the CU.
//
// The 3x3 part is the family's stride-2 form (hreg_core.h: HrS2), a wave's weights in registers (72 per 16-cout fragment; with C3 = 128 a
// wave holds fragments `wave` and `wave + 4`: one workgroup stages the halo once where the layer-by-layer launch staged it in two).
// Each accumulator is summed as in conv3x3_hreg_s2_kernel: from the bias, then chunk, halo row, kernel row, column.
// The hand-over is conv3x3_hc2f.hip's `mid` image: SiLU, ONE rounding to the storage type, [chunk C3 / 32][row 4][pixel 16] x 64 B with the
// halo's part swizzle.  The 1x1 runs on MFMAs with a wave owning two 16-cout fragments and the tile's 4 rows, K ascending from a zero
// accumulator, bias last (conv1x1_stream's summation): the launch computes what its two launches compute, bit for bit.  Its weights are
// resident per wave (a wave owns 32 couts and K is 128 / 192): form B 48 registers; form A 16 registers + 16 KB of LDS for the workgroup
// (see NW1R below: its 3x3 weights alone are 144 registers).
//
// Items of a tile: the two halo chunks, then (form B) the CENTRE pixels of the two 64-channel groups of `other` (64 pixels x 64 channels
// = 8 KB, DMA'd straight into mid's format).  Form A: ring of two stages, the DMA one item ahead; `mid` is published by a barrier of its
// own inside the tile's second item and the 1x1 follows it.  Form B: ring of three stages, two items ahead; `mid` is published by the
// barrier that ends the second item and read in the third.  Every item ends with the family's full drain + barrier, and all output stores
// of a tile leave back to back behind the epilogue's arithmetic (hreg_core.h: the drain rule, the store rule).
#include "common_hip.h"
#include "hreg_core.h"

namespace DY_NS {

struct HdownArgs {
  const void* x;      // 3x3 input, NHWC (N, H, W, 64), pitch ldx
  const void* w3;     // 3x3 64 -> C3, DY_WLAYOUT_HALO3X3 (NF = 4, C3 / 64 cout tiles)
  const float* b3;    // C3
  const void* other;  // form B: NHWC (N, Ho, Wo, 128), pitch ldo
  const void* w1;     // 1x1 (C3 + NOG * 64) -> 128, DY_WLAYOUT_FRAG1X1 (NF = 8)
  const float* b1;    // 128
  void* y;            // NHWC (N, Ho, Wo, 128), pitch ldy
  int N, H, W, ldx, ldo, ldy;
  unsigned x_bytes, o_bytes, y_bytes;
  int tilesX, tilesY, nSpatial;
};

constexpr int kHdTH = HrS2::TH, kHdTW = HrS2::TW, kHdStage = HrS2::kStage;
constexpr int kHdChunk = kHdTH * kHdTW * 64;  // 4 KB: one 32-channel chunk of `mid` / of an operand image

template <typename T, int C3, int NOG>
__global__ __launch_bounds__(256, 2) void conv3x3_hdown_kernel(const HdownArgs p) {
  static_assert((C3 == 128 && NOG == 0) || (C3 == 64 && NOG == 2), "built for the two forms of Drone-YOLO-s");
  constexpr int EPC = Elem<T>::EPC;  // 8
  constexpr int NCH = 2, NIT = NCH + NOG;          // items per tile: halo chunks, operand groups
  constexpr int NF3 = C3 / 64;                     // 16-cout fragments of the 3x3 a wave holds
  constexpr int NST = NOG ? 3 : 2, LA = NST - 1;   // ring stages; the loader runs LA items ahead
  constexpr int NKM = C3 / 32, NKG = NKM + NOG * 2;  // k-groups (32 channels) of the 1x1: `mid`, all
  constexpr int NF1 = 8;                           // 16-cout fragments per k-group of the 1x1 image (cout 128)
  constexpr int kMid = NKM * kHdChunk;
  // Registers.  Form B: everything resident (72 + 48 weight registers).  Form A's 3x3 weights alone are 144, so of its 1x1 only NW1R
  // k-groups stay in registers, the rest waits in the 16 KB of LDS the two-stage ring leaves below 80 KB, and the biases are fetched per
  // tile where the accumulators they go with are dead (resident: 256 registers and 25 spilled).
  constexpr int NW1R = NOG ? NKG : 2;
  constexpr bool BIAS_RES = NOG > 0;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[NST * kHdStage + kMid + (NKG - NW1R) * NF1 * 1024];
  unsigned char* const mid = smem + NST * kHdStage;
  unsigned char* const w1s = mid + kMid;  // [k-group - NW1R][fragment 8] x 1 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane >> 4, lr = lane & 15;
  const int Ho = (p.H - 1) / 2 + 1, Wo = (p.W - 1) / 2 + 1;

  const int G = (int)gridDim.x;
  const int sb = hr_block(G, 1).sb;
  const int myTiles = hr_my_tiles(p.nSpatial, sb, G);
  if (myTiles <= 0) return;
  const int nItems = myTiles * NIT;

  // ---- register-resident weights: the wave's fragments of the 3x3 (`wave` of every 64-cout tile) and of the 1x1 (2 wave, 2 wave + 1) ----
  u32x4 wreg[NF3][NCH][9];
#pragma unroll
  for (int f = 0; f < NF3; ++f) hr_load_wreg<NCH>(wreg[f], reinterpret_cast<const u32x4*>(p.w3) + f * NCH * 9 * 4 * 64, wave, lane);
  u32x4 w1[NW1R][2];
  {
    const u32x4* wg = reinterpret_cast<const u32x4*>(p.w1);
#pragma unroll
    for (int g = 0; g < NW1R; ++g)
#pragma unroll
      for (int f = 0; f < 2; ++f) w1[g][f] = wg[(g * NF1 + wave * 2 + f) * 64 + lane];
    for (int i = tid; i < (NKG - NW1R) * NF1 * 64; i += 256)  // (published by the barrier that opens the item pipeline)
      *reinterpret_cast<u32x4*>(w1s + i * 16) = wg[NW1R * NF1 * 64 + i];
  }
  // the biases of a lane's accumulator rows: 3x3 fragment f -> b3[f * 64 + wave * 16 + lq * 4 ..], 1x1 fragment f -> b1[(wave * 2 + f) * 16 + lq * 4 ..]
  const __amdgpu_buffer_rsrc_t b3rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.b3), 0, C3 * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t b1rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.b1), 0, 128 * 4, 0x00020000);
  const int b3off = (wave * 16 + lq * 4) * 4, b1off = (wave * 32 + lq * 4) * 4;
  f32x4 bias3[NF3], bias1[2];
  auto load_bias3 = [&]() {
#pragma unroll
    for (int f = 0; f < NF3; ++f) bias3[f] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b3rs, b3off, f * 256, 0));
  };
  auto load_bias1 = [&]() {
#pragma unroll
    for (int f = 0; f < 2; ++f) bias1[f] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b1rs, b1off, f * 64, 0));
  };
  load_bias3();
  if constexpr (BIAS_RES) load_bias1();

  // ---- loaders ----
  constexpr unsigned kOob = kHrOob;
  constexpr int NDMA = HrS2::NDMA;        // halo: 6 wave-instructions per wave and item (1 KB each: w, w + 4, .., w + 20)
  constexpr int NDMO = 2;                 // operand group: 2 (block i = k * 4 + wave is chunk k, row wave)
  const unsigned pre = (unsigned)((p.W + 1) * p.ldx) * 2u;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.x)) - pre, 0, p.x_bytes + pre, 0x00020000);
  const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(NOG ? p.other : p.x), 0, NOG ? p.o_bytes : 0u, 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.y_bytes, 0x00020000);
  unsigned rel[NDMA];  // launch constants: ((hy W + hx) ldx + part') * 2
  hr_halo_rel<HrS2>(rel, wave, lane, p.W, p.ldx, 2u, 2u * EPC);
  unsigned orel[NDMO];  // operand: ((row Wo + pixel) ldo + chunk * 32 + part' * 8) * 2
#pragma unroll
  for (int k = 0; k < NDMO; ++k) {
    const int px = lane >> 2;
    orel[k] = (unsigned)((wave * Wo + px) * p.ldo + k * 4 * EPC + ((lane & 3) ^ ((px >> 1) & 3)) * EPC) * 2u;
  }
  unsigned l_base_x = 0, l_base_o = 0;
  bool l_interior = false;   // the loader's tile needs no zero padding (wave-uniform)
  int l_y0 = 0, l_x0 = 0;    // input coordinates of the centre tap of its first output pixel
  int l_oy0 = 0, l_ox0 = 0;  // output coordinates of the loader's tile
  int l_tile = sb, l_item = 0;
  auto setup_tile = [&](int tile) {
    const HrTile t = hr_tile(tile, p.tilesX, p.tilesY);
    l_oy0 = t.ty * kHdTH, l_ox0 = t.tx * kHdTW;
    l_y0 = 2 * l_oy0, l_x0 = 2 * l_ox0;
    l_base_x = (unsigned)(((t.n * p.H + l_y0) * p.W + l_x0) * p.ldx) * 2u;
    if constexpr (NOG > 0) l_base_o = (unsigned)(((t.n * Ho + l_oy0) * Wo + l_ox0) * p.ldo) * 2u;
    l_interior = hr_interior<HrS2>(l_y0, l_x0, p.H, p.W);
  };
  // DMA of the loader's item into `stage`, then advance the loader.  `kind` is the item's place in its tile (a compile-time constant at
  // every call: the loader runs exactly LA items ahead of the compute).
  auto issue_dma = [&](int stage, int kind) {
    if (l_item >= nItems) return;  // (wave-uniform)
    unsigned char* sa = smem + stage * kHdStage;
    if (kind < NCH) {
      const unsigned soff = l_base_x + (unsigned)kind * (4u * EPC * (unsigned)sizeof(T));
      if (l_interior) {
        hr_issue<NDMA>(xrs, sa, wave, rel, soff);
      } else {  // border tile: out-of-image slots get an out-of-range offset (zeros); worked out per item, not kept in six more registers
#pragma unroll
        for (int k = 0; k < NDMA; ++k) hr_issue1(xrs, sa, k, wave, hr_halo_inside<HrS2>(k, wave, lane, l_y0, l_x0, p.H, p.W) ? rel[k] : kOob, soff);
      }
    } else {
      const unsigned soff = l_base_o + (unsigned)(kind - NCH) * (64u * (unsigned)sizeof(T));
      const bool whole = l_oy0 + kHdTH <= Ho && l_ox0 + kHdTW <= Wo;  // wave-uniform
#pragma unroll
      for (int k = 0; k < NDMO; ++k) {
        unsigned vo = orel[k];
        if (!whole) vo = (l_oy0 + wave < Ho && l_ox0 + (lane >> 2) < Wo) ? vo : kOob;
        hr_issue1(ors, sa, k, wave, vo, soff);
      }
    }
    ++l_item;
    if (kind == NIT - 1) {
      l_tile += G;
      if (l_item < nItems) setup_tile(l_tile);
    }
  };

  int lane_base[3];  // ([0] also: pixel lr, part lq of a `mid` / operand row)
  HrS2::lane_base(lane_base, lr, lq);

  f32x4 acc[NF3][kHdTH];  // 3x3: NF3 x 16 couts x (4 rows x 16 pixels)
  f32x4 acc1[2][kHdTH];   // 1x1: 2 x 16 couts x (4 rows x 16 pixels)

  // 1x1 over one 64-channel operand image (a ring stage or two chunks of `mid`), weights w1[g0], w1[g0 + 1]: one fragment read feeds both
  // of the wave's cout fragments
  auto gemm1 = [&](const unsigned char* img, int g0) {
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
      for (int o = 0; o < kHdTH; ++o) {
        const u32x4 b = *reinterpret_cast<const u32x4*>(img + lane_base[0] + c2 * kHdChunk + o * (kHdTW * 64));
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          u32x4 w;
          if (g0 + c2 < NW1R) w = w1[g0 + c2 < NW1R ? g0 + c2 : 0][f];
          else w = *reinterpret_cast<const u32x4*>(w1s + ((g0 + c2 - NW1R) * NF1 + wave * 2 + f) * 1024 + lane * 16);
          acc1[f][o] = Elem<T>::mma(w, b, acc1[f][o]);
        }
      }
  };
  auto gemm1_mid = [&]() {  // ascending K from a zero accumulator: the 3x3's output is the 1x1's first C3 channels
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int o = 0; o < kHdTH; ++o) acc1[f][o] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < NKM; g += 2) gemm1(mid + g * kHdChunk, g);
  };

  const int mid_w = hr_mid_offset(wave, lr, lq, kHdChunk);  // + f * 2 chunks + o * 1024: fragment f holds channels (f * 4 + wave) * 16 + lq * 4 .. + 3
  // the 3x3's epilogue: SiLU, ONE rounding to the storage type, into `mid`
  auto tail_mid = [&]() {
#pragma unroll
    for (int f = 0; f < NF3; ++f) hr_tail_mid<T, kHdTH, false>(acc[f], mid + mid_w + f * (2 * kHdChunk), nullptr);
  };

  // output: quarter lq stores channels f * 16 + 8 (lq >> 1) .. + 7 of the wave's 32, row o + (lq & 1), column lr
  unsigned lane_out[kHdTH / 2];
  hr_lane_out<kHdTH>(lane_out, lr, lq, Wo, p.ldy, wave * 32 + (lq >> 1) * 8, (unsigned)sizeof(T));
  auto epilogue = [&](int tile) {
    const HrTile t = hr_tile(tile, p.tilesX, p.tilesY);
    const int y0 = t.ty * kHdTH, x0 = t.tx * kHdTW;  // output coordinates
    const unsigned out_base = (unsigned)(((t.n * Ho + y0) * Wo + x0) * p.ldy) * (unsigned)sizeof(T);  // scalar
    hr_out_1x1<T, kHdTH>(acc1, bias1, lane_out, yrs, out_base, y0, x0, Ho, Wo, lr, lq);
  };
  auto finish = [&](int tile) {
    hr_settle_mfma();
    epilogue(tile);
  };

  // ---- item pipeline: item i lives in stage i % NST; at its start the DMA of item i + LA goes into the stage last read in item i - 1
  // (every wave has passed the barrier that ended it); one drain + barrier per item ----
  setup_tile(l_tile);
#pragma unroll
  for (int i = 0; i < LA; ++i) issue_dma(i, i);
  __builtin_amdgcn_s_waitcnt(kHrVmcnt0);
  __syncthreads();
  int c_tile = sb;
  int stage = 0;
  for (int it = 0; it < nItems; it += NIT) {
#pragma unroll
    for (int kind = 0; kind < NIT; ++kind) {
      issue_dma(stage + LA >= NST ? stage + LA - NST : stage + LA, (kind + LA) % NIT);
      const unsigned char* sa = smem + stage * kHdStage;
      if (kind < NCH) {
        if (kind == 0) {
#pragma unroll
          for (int f = 0; f < NF3; ++f)
#pragma unroll
            for (int o = 0; o < kHdTH; ++o) acc[f][o] = bias3[f];
        }
        hr_rows_s2<T, NF3, NCH>(acc, wreg, sa, lane_base, kind);
        if (kind == NCH - 1) {
          tail_mid();
          if constexpr (NOG == 0) {  // `mid` published inside the item: every wave reads all of its channels
            load_bias1();  // (the 3x3's accumulators are dead: no register the main loop needs; back long before the epilogue)
            load_bias3();  // for the next tile's accumulators (in front of the tile's output stores: nothing but the drain follows those)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            gemm1_mid();
            finish(c_tile);
            c_tile += G;
          }
        }
      } else {
        const int j = kind - NCH;
        if (j == 0) gemm1_mid();  // (the Concat's first source)
        gemm1(sa, NKM + 2 * j);
        if (j == NOG - 1) {
          finish(c_tile);
          c_tile += G;
        }
      }
      __builtin_amdgcn_s_waitcnt(kHrVmcnt0);
      __syncthreads();  // the ring's next image complete and visible; `mid` written; the output stores retired
      stage = stage + 1 == NST ? 0 : stage + 1;
    }
  }
}

template <typename T>
static int launch_hdown(const HdownArgs& a, bool form_b, hipStream_t st) {
  const int grid = hr_grid(2, a.nSpatial, 1);  // two 256-thread workgroups per CU (64 / 80 KB of LDS each)
  const dim3 g((unsigned)grid), b(256);
  if (form_b) hipLaunchKernelGGL((conv3x3_hdown_kernel<T, 64, 2>), g, b, 0, st, a);
  else hipLaunchKernelGGL((conv3x3_hdown_kernel<T, 128, 0>), g, b, 0, st, a);
  return check_launch("conv3x3_hdown_kernel");
}

}  // namespace DY_NS

using namespace DY_NS;

#ifndef DYOLO_L2E_BUILD
extern "C" int32_t dy_c2f_front_fused_supported(int32_t cin, int32_t cmid, int32_t c_other, int32_t cout, int32_t ksize, int32_t stride, int32_t groups, int32_t act,
                                                int32_t dtype) {
  if (!(dtype == DY_BF16 || dtype == DY_F16)) return 0;
  if (!(act == DY_ACT_SILU || act == DY_ACT_SILU_L2E)) return 0;
  const bool form_a = cmid == 128 && c_other == 0, form_b = cmid == 64 && c_other == 128;
  return cin == 64 && (form_a || form_b) && cout == 128 && ksize == 3 && stride == 2 && groups == 1;
}

namespace dy_l2e {
int32_t c2f_front_entry(const dy_c2f_front_desc* d, dy_stream_t stream);
}
namespace dy {
int32_t c2f_front_entry(const dy_c2f_front_desc* d, dy_stream_t stream);
}
extern "C" int32_t dy_c2f_front_fused(const dy_c2f_front_desc* d, dy_stream_t stream) {
  return (d != nullptr && d->act == DY_ACT_SILU_L2E) ? dy_l2e::c2f_front_entry(d, stream) : dy::c2f_front_entry(d, stream);
}
#endif

namespace DY_NS {
int32_t c2f_front_entry(const dy_c2f_front_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->x && d->y && d->w3 && d->b3 && d->w1 && d->b1, DY_ERR_INVALID_ARG, "dy_c2f_front_fused: null pointer");
  DY_REQUIRE(dy_c2f_front_fused_supported(d->cin, d->cmid, d->c_other, d->cout, 3, 2, 1, d->act, d->dtype), DY_ERR_UNSUPPORTED,
             "dy_c2f_front_fused: built for a 3x3 stride-2 SiLU convolution 64 -> 128 (no second source) or 64 -> 64 (+ 128 channels), cout 128, 16-bit storage "
             "(got %d -> %d + %d -> %d act %d dtype %d): run the two dy_conv2d_nhwc calls",
             d->cin, d->cmid, d->c_other, d->cout, d->act, d->dtype);
  const bool form_b = d->c_other > 0;
  DY_REQUIRE(!form_b || d->other, DY_ERR_INVALID_ARG, "dy_c2f_front_fused: null pointer (other)");
  DY_REQUIRE(d->batch > 0 && d->h > 0 && d->w > 0 && d->ld_x >= d->cin && (!form_b || d->ld_other >= d->c_other) && d->ld_y >= d->cout, DY_ERR_INVALID_ARG,
             "dy_c2f_front_fused: bad dims / pitches");
  DY_REQUIRE(d->ld_x % 8 == 0 && d->ld_y % 8 == 0 && (!form_b || (d->ld_other % 8 == 0 && aligned16(d->other))) && aligned16(d->x) && aligned16(d->y) && aligned16(d->w3) &&
                 aligned16(d->w1) && aligned16(d->b3) && aligned16(d->b1),
             DY_ERR_INVALID_ARG, "dy_c2f_front_fused: views must be whole 16-byte chunks");
  const int ho = (d->h - 1) / 2 + 1, wo = (d->w - 1) / 2 + 1;
  const long long pin = (long long)d->batch * d->h * d->w, pout = (long long)d->batch * ho * wo;
  DY_REQUIRE(pin * d->ld_x * 2 < (1ll << 31) && (!form_b || pout * d->ld_other * 2 < (1ll << 31)) && pout * d->ld_y * 2 < (1ll << 32) - 64, DY_ERR_UNSUPPORTED,
             "dy_c2f_front_fused: a view exceeds 2 GiB (32-bit offsets)");
  HdownArgs a{};
  a.x = d->x, a.w3 = d->w3, a.b3 = d->b3, a.other = form_b ? d->other : nullptr, a.w1 = d->w1, a.b1 = d->b1, a.y = d->y;
  a.N = d->batch, a.H = d->h, a.W = d->w, a.ldx = d->ld_x, a.ldo = form_b ? d->ld_other : 0, a.ldy = d->ld_y;
  a.x_bytes = (unsigned)(pin * d->ld_x * 2), a.o_bytes = form_b ? (unsigned)(pout * d->ld_other * 2) : 0u, a.y_bytes = (unsigned)(pout * d->ld_y * 2);
  a.tilesX = (wo + kHdTW - 1) / kHdTW, a.tilesY = (ho + kHdTH - 1) / kHdTH;
  a.nSpatial = d->batch * a.tilesX * a.tilesY;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return d->dtype == DY_BF16 ? launch_hdown<bf16_t>(a, form_b, st) : launch_hdown<f16_t>(a, form_b, st);
}
}  // namespace DY_NS
