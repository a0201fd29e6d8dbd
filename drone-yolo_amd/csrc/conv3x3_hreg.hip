// 3x3 pad-1 NHWC convolution for the narrow 16-bit layers (cin 64 / 128, cout a multiple of 64) with the weights held in REGISTERS
// (hreg_core.h describes the decomposition, the image, the loader and the two rules): the kernel the 64->64 layers of the model run on
// (the P2 Detect trunks, the stride-8 C2f Bottlenecks: 18 launches, the largest share of a pass), at stride 1 and stride 2.
//
// Why another 3x3 kernel.  conv3x3_halo.hip keeps the layer's weights stationary in LDS (72 KB for 64->64) and every
// wave re-reads them per tap: 0.75 LDS reads per MFMA, one 512-thread workgroup per CU (LDS capacity), two waves per
// SIMD that run in barrier lock-step.  Its counters (profiles/r01_pmc_halo_64x64_3x3_80.txt) show no unit saturated:
// matrix pipe 37 % busy, 37 % of the wave cycles parked in s_waitcnt / s_barrier, 27 % of the LDS cycles lost to bank
// conflicts of the 80-byte pixel pitch.  This kernel changes the decomposition instead of the schedule: a ring of three halo stages
// (stride 1: 16 KB each, three workgroups per CU; stride 2: 24 KB, two), 30 ds_read_b128 per 72 MFMAs = 0.42 reads per MFMA instead of 0.75,
// and the result (bias-initialised accumulator, SiLU, optional Bottleneck residual) stored straight from registers.
//
// One raw s_barrier per (tile, chunk) item.  The DMA of item i + 2 is issued at the start of item i and drained before the barrier that ends it.
//
// Stride 2 (r03): the 64-channel DOWNSAMPLING layers (64->128 @160 of the backbone, 64->64 @160 of the neck) ran on the flat-M LDS-DMA GEMM
// with a per-tap gather (399 / 597 TFLOP/s: every input pixel crossed the L2->LDS path 2.25 times and a 128 x 64 tile with K = 576 is nine
// short steps between a prologue and an epilogue).  With the two column-parity planes of HrS2 a wave walks the 9 halo rows per chunk:
// 36 MFMAs per 27 reads.
// Reference semantics: Conv (nn/modules/conv.py:37-55, BatchNorm folded), Bottleneck shortcut (block.py:337-350).
#include "common_hip.h"
#include "conv_args.h"
#include "hreg_core.h"

namespace DY_NS {


struct HregArgs {
  const void* x;
  const void* w;       // DY_WLAYOUT_HALO3X3 packing with NF = 4: 1 KB blocks [(nt * nChunks + chunk) * 9 + tap][j], lane-major
  const float* bias;   // cout_pad floats
  const void* res;
  void* y;
  int N, H, W, Cin, ldx, Cout, ldy, ldres, act;
  int tilesX, tilesY, tilesN, nSpatial;  // spatial tiles (n, ty, tx) and 64-cout groups
  unsigned x_bytes, y_bytes, r_bytes;
  double* stats;  // optional: a dy_bn_train_fwd workspace; spatial block sb stores its per-channel sum / sum of squares of the STORED outputs in slot sb (dy_conv_desc.bn_stats)
  const float* bnb_mean;  // BNB (dy_conv_desc.bnb_z, which travels as `res`): the BatchNorm in front of the layer whose gradient this launch computes
  const float* bnb_rstd;
  const float* bnb_gamma;
  const float* bnb_beta;
  int bnb_act;
  int dbg;  // -DDYOLO_ABLATE builds only (DYOLO_DBG): 1 no output stores, 2 no MFMAs, 4 no DMA after the prologue, 8 no fragment reads
};

#ifdef DYOLO_ABLATE
#define HR_DBG(bit) (p.dbg & (bit))
#else
#define HR_DBG(bit) 0
#endif

constexpr int kHrStages = 3;

// STATS: training forward (the convolution in front of a train-mode BatchNorm, conv.py:49-51): the batch statistics of the stored
// output come out of the epilogue -- a lane always holds the same four output channels, so it keeps their sums over all of its tiles
// in 8 registers and the kernel ends with one shuffle reduction over the 16 pixel lanes and 32 plain stores per wave into the
// workgroup's slot of the BatchNorm workspace (dy_bn_train_fwd adds the slots up as it does for its own reduction pass; atomics on
// the 2 x Cout totals from ~770 workgroups serialise: +0.7 ms per step, measured) -- instead of a separate pass that reads the whole
// map again (dy_bn_train_fwd's reduction: 1.4 of 10 ms of BatchNorm per step at B = 64).
// BNB (r05; training backward, dy_conv_desc.bnb_z): the launch computes the gradient dy that reaches the BatchNorm + activation of the layer
// in front, and that BatchNorm's backward needs sum(du) and sum(du xhat) over the batch before it can form dz (du = dy act'(u), u = gamma xhat
// + beta, xhat = (z - mean) rstd) -- a pass of its own over dy and z (dy_bn_train_bwd's reduction: 2.8 of 8.9 ms of BatchNorm per step at
// B = 64).  Here the tile's z arrives the way a residual does (16 bytes per lane and row pair, requested an item ahead), the epilogue forms du
// from the STORED dy, and the sums leave through the STATS slots.  A gradient convolution has no activation, so the epilogue's vector issue
// is free where the forward kernel spends it on SiLU.
// The four BatchNorm constants per channel (rstd, -mean rstd, gamma rstd, beta - gamma rstd mean) wait in 1 KB of LDS and are read in the
// epilogue only: in registers they cost the main loop 16 of its 168 (64 channels) / 256 (128 channels) and spilled 38 / 22.
// One body for both geometries (Geom = HrS1 / HrS2; RES and BNB are built at stride 1 only).
template <typename T, typename Geom, int NCH, bool RES, bool STATS, bool BNB>
__device__ __forceinline__ void hreg_body(const HregArgs& p) {
  static_assert(!(BNB && (RES || STATS)), "BNB: its own mode");
  static_assert(Geom::kStride == 1 || !(RES || BNB), "stride 2: no residual, no BNB");
  constexpr bool SLOTS = STATS || BNB, RLOAD = RES || BNB;
  constexpr int EPC = Elem<T>::EPC;  // 8
  constexpr int TH = Geom::TH, TW = Geom::TW, NDMA = Geom::NDMA;  // every wave issues exactly NDMA wave-instructions per item (w, w + 4, ..)
  __shared__ __attribute__((aligned(1024))) unsigned char smem[kHrStages * Geom::kStage];
  __shared__ f32x4 bnc[BNB ? 64 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane >> 4, lr = lane & 15;
  const int Ho = (p.H - 1) / Geom::kStride + 1, Wo = (p.W - 1) / Geom::kStride + 1;
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.y_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.res ? p.res : p.y), 0, p.res ? p.r_bytes : 0u, 0x00020000);

  // block -> (cout group, spatial sequence)
  const HrBlock blk = hr_block((int)gridDim.x, p.tilesN);
  const int nt = blk.nt, sb = blk.sb, Gs = blk.Gs;
  const int myTiles = hr_my_tiles(p.nSpatial, sb, Gs);
  if constexpr (SLOTS) hr_stats_zero(p.stats, p.Cout, nt, sb, tid, myTiles > 0);
  if (myTiles <= 0) return;
  const int nItems = myTiles * NCH;

  u32x4 wreg[1][NCH][9];
  hr_load_wreg<NCH>(wreg[0], reinterpret_cast<const u32x4*>(p.w) + (size_t)nt * NCH * 9 * 4 * 64, wave, lane);
  const f32x4 bias4 = *reinterpret_cast<const f32x4*>(p.bias + nt * 64 + wave * 16 + lq * 4);

  // ---- loader: this kernel keeps the slots' halo pixels in a table (hy | hx << 8) for its border tiles ----
  const unsigned pre = (unsigned)((p.W + 1) * p.ldx) * 2u;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p.x)) - pre, 0, p.x_bytes + pre, 0x00020000);
  unsigned rel[NDMA];  // launch constants
  int hyx[NDMA];
  hr_halo_rel<Geom>(rel, wave, lane, p.W, p.ldx, 2u, 2u * EPC);
#pragma unroll
  for (int k = 0; k < NDMA; ++k) {
    int hy, hx, key;
    Geom::slot(k, wave, lane, hy, hx, key);
    hyx[k] = hy | (hx << 8);
  }
  unsigned voff[NDMA];  // this lane's offsets for the loader's current tile
  unsigned l_base = 0;  // scalar: byte offset of the centre tap of the tile's first output pixel in image n, in the shifted descriptor's terms the tile's halo origin
  int l_tile = sb, l_chunk = 0, l_item = 0;
  auto setup_tile = [&](int tile) {
    const HrTile t = hr_tile(tile, p.tilesX, p.tilesY);
    const int y0 = Geom::kStride * t.ty * TH, x0 = Geom::kStride * t.tx * TW;
    l_base = (unsigned)(((t.n * p.H + y0) * p.W + x0) * p.ldx) * 2u;
    if (hr_interior<Geom>(y0, x0, p.H, p.W)) {
#pragma unroll
      for (int k = 0; k < NDMA; ++k) voff[k] = rel[k];
    } else {
#pragma unroll
      for (int k = 0; k < NDMA; ++k) {
        const int gy = y0 - 1 + (hyx[k] & 255), gx = x0 - 1 + (hyx[k] >> 8);
        voff[k] = ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) ? rel[k] : kHrOob;
      }
    }
  };
  auto issue_dma = [&](int stage) {  // DMA of item (l_tile, l_chunk) into `stage`, then advance the loader; past the last item: zeros
    unsigned char* sa = smem + stage * Geom::kStage;
    const bool live = l_item < nItems && !(HR_DBG(4) && l_item >= 2);
    if (live) {
      hr_issue<NDMA>(xrs, sa, wave, voff, l_base + (unsigned)l_chunk * (4u * EPC * (unsigned)sizeof(T)));
      ++l_item;
      if (++l_chunk == NCH) {
        l_chunk = 0;
        l_tile += Gs;
        if (l_item < nItems) setup_tile(l_tile);
      }
    } else {
#pragma unroll
      for (int k = 0; k < NDMA; ++k) hr_issue1(xrs, sa, k, wave, kHrOob, 0u);  // keeps the per-item instruction count — every lane out of range: zeros
    }
  };

  int lane_base[3];
  Geom::lane_base(lane_base, lr, lq);

  f32x4 acc[1][TH];
#pragma unroll
  for (int o = 0; o < TH; ++o) acc[0][o] = bias4;

  auto compute = [&](int stg, int c) {
    const unsigned char* sa = smem + stg * Geom::kStage;
    if constexpr (Geom::kStride == 1) hr_rows_s1<T, NCH>(acc[0], wreg[0], sa, lane_base, c, HR_DBG(2 | 8));
    else hr_rows_s2<T, 1, NCH>(acc, wreg, sa, lane_base, c);
  };

  // residual of the tile that ends with this item (Bottleneck shortcut): requested at the START of the item, BEFORE the next
  // DMA is issued — the loads are then older than that DMA and their wait (at the epilogue) leaves it in flight
  typedef __attribute__((ext_vector_type(4))) T t4;
  u32x4 rl[TH / 2];  // 16 bytes per lane and row pair, in the store order of the epilogue (quarter lq: row o + (lq & 1), channels 8 (lq >> 1) ..)
  const int co16 = nt * 64 + wave * 16 + (lq >> 1) * 8;
  auto load_residual = [&](int tile) {
    const HrTile t = hr_tile(tile, p.tilesX, p.tilesY);
    const int xx = t.tx * TW + lr;
#pragma unroll
    for (int o = 0; o < TH; o += 2) {
      const int yy = t.ty * TH + o + (lq & 1);
      const bool ok = yy < p.H && xx < p.W;
      const unsigned off = ok ? (unsigned)((((size_t)(t.n * p.H + yy) * p.W + xx) * (size_t)p.ldres + co16) * sizeof(T)) : kHrOob;
      rl[o / 2] = __builtin_amdgcn_raw_buffer_load_b128(rrs, off, 0, 0);
    }
  };
  // store offsets: lane constant (row o + (lq & 1) of the pair, column lr, 8 channels from co16) + a scalar tile offset (soffset)
  unsigned lane_out[TH / 2];
  hr_lane_out<TH>(lane_out, lr, lq, Wo, p.ldy, co16, (unsigned)sizeof(T));
  float st_sum[4] = {0.f, 0.f, 0.f, 0.f}, st_sq[4] = {0.f, 0.f, 0.f, 0.f};  // STATS: this lane's four channels, all its tiles
  if constexpr (BNB) {  // (published by the barrier that opens the item pipeline)
    if (tid < 64) {
      const int co = nt * 64 + tid;
      const float mu = p.bnb_mean[co], rs = p.bnb_rstd[co], gr = p.bnb_gamma[co] * rs;
      bnc[tid] = f32x4{rs, -mu * rs, gr, p.bnb_beta[co] - gr * mu};
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  // The store rule, in this kernel's form (hreg_core.h): the stores leave among the epilogue's arithmetic, as they always did here, and their
  // data registers `st` stay live until the item's drain has retired them (hr_hold behind it)
  u32x4 st[TH / 2];
  auto epilogue = [&](int tile) {
    const HrTile t = hr_tile(tile, p.tilesX, p.tilesY);
    const int y0 = t.ty * TH, x0 = t.tx * TW;  // output coordinates
    const unsigned out_base = (unsigned)(((t.n * Ho + y0) * Wo + x0) * p.ldy) * (unsigned)sizeof(T);  // scalar
    const bool whole = y0 + TH <= Ho && x0 + TW <= Wo;                                                 // wave-uniform: no ragged edge
    u32x2 pk[TH];
#pragma unroll
    for (int o = 0; o < TH; ++o) {
      float v[4] = {acc[0][o][0], acc[0][o][1], acc[0][o][2], acc[0][o][3]};
      if (p.act == DY_ACT_SILU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = silu_f32(v[e]);
      }
      if constexpr (RES) {
        const t4 rr = __builtin_bit_cast(t4, hr_unpack_pair(rl[o / 2], o & 1));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += Elem<T>::to_f32(rr[e]);
      }
      t4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = Elem<T>::from_f32(v[e]);
      if constexpr (STATS) {
        if (whole || (y0 + o < Ho && x0 + lr < Wo)) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float f = Elem<T>::to_f32(ov[e]);  // what BatchNorm will read back
            st_sum[e] += f, st_sq[e] += f * f;
          }
        }
      }
      if constexpr (BNB) {
        const t4 zz = __builtin_bit_cast(t4, hr_unpack_pair(rl[o / 2], o & 1));  // z of this lane's pixel and channels, as RES reads its residual
        if (whole || (y0 + o < Ho && x0 + lr < Wo)) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f32x4 k = bnc[wave * 16 + lq * 4 + e];
            const float zf = Elem<T>::to_f32(zz[e]);
            const float xh = zf * k[0] + k[1];
            float du = Elem<T>::to_f32(ov[e]);  // the gradient as the BatchNorm's apply pass will read it back
            if (p.bnb_act == DY_ACT_SILU) {
              const float u = zf * k[2] + k[3];
              const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * -1.4426950408889634f));
              du *= sg * (1.0f + u * (1.0f - sg));  // bn_train.hip: silu_grad
            }
            st_sum[e] += du, st_sq[e] += du * xh;
          }
        }
      }
      pk[o] = __builtin_bit_cast(u32x2, ov);
      acc[0][o] = bias4;
    }
#pragma unroll
    for (int o = 0; o < TH; o += 2) {
      st[o / 2] = hr_pack_pair(pk[o], pk[o + 1]);
      unsigned off = lane_out[o / 2];
      if (!whole) off = (y0 + o + (lq & 1) < Ho && x0 + lr < Wo) ? off : kHrOob;
      __builtin_amdgcn_raw_buffer_store_b128(st[o / 2], yrs, HR_DBG(1) ? kHrOob : off, (int)out_base, 0);
    }
  };

  // ---- item pipeline: ring of three stages, raw barriers ----
  // Item i lives in stage i % 3.  At the start of item i the DMA of item i + 2 goes into stage (i + 2) % 3, last read in
  // item i - 1 (every wave has passed the barrier that ended it).  At the end of item i the wave drains its vector-memory
  // operations (vmcnt(0): its pieces of items i + 1 and i + 2, and the tile's output stores); the barrier then publishes
  // everyone's pieces.  (Counted waits that left item i + 2 in flight were not safe: the drain rule.)
  setup_tile(l_tile);
  issue_dma(0);
  issue_dma(1 % kHrStages);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  int c_tile = sb;
  int stage = 0;
  for (int it = 0; it < nItems; it += NCH) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if constexpr (RLOAD) {
        if (c == NCH - 1) load_residual(c_tile);
      }
      issue_dma(stage + 2 >= kHrStages ? stage + 2 - kHrStages : stage + 2);
      compute(stage, c);
      if (c == NCH - 1) {
        epilogue(c_tile);
        c_tile += Gs;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (c == NCH - 1) hr_hold(st);
      __builtin_amdgcn_s_barrier();
      stage = stage + 1 == kHrStages ? 0 : stage + 1;
    }
  }
  if constexpr (SLOTS) hr_stats_store(p.stats, p.Cout, nt, sb, wave, lq, lr, st_sum, st_sq);
}

// BW: workgroups per CU the 64-channel BNB form is compiled for (3: 168 registers, 29 spilled; 2: 198, none).
template <typename T, int NCH, bool RES, bool STATS = false, bool BNB = false, int BW = 3>
__global__ __launch_bounds__(256, NCH <= 2 ? (BNB ? BW : 3) : 2) void conv3x3_hreg_kernel(const HregArgs p) {
  hreg_body<T, HrS1, NCH, RES, STATS, BNB>(p);
}

template <typename T, int NCH, bool STATS = false>  // STATS: as in the stride-1 kernel (r04)
__global__ __launch_bounds__(256, 2) void conv3x3_hreg_s2_kernel(const HregArgs p) {
  hreg_body<T, HrS2, NCH, false, STATS, false>(p);
}

[[maybe_unused]] constexpr int kBnbWgs = 2;  // measured (tools/bn_behind_ab.sh, B = 64 step): 3 per CU with 29 spills +0.2 ms, 2 per CU without -0.1 ms against the two-pass form
template <typename T>
static int launch_hreg(const HregArgs& a, hipStream_t st) {
  HregArgs p = a;
  const int nch = p.Cin / 32;
  // three 256-thread workgroups per CU (48 KB of LDS and <= 168 VGPRs each); r04, 128 input channels (four chunks: 144 weight registers):
  // two per CU with up to 256 registers
  const long long nwork = (long long)p.nSpatial * p.tilesN;
  int grid = hr_grid(nch <= 2 ? 3 : 2, nwork, p.tilesN);
  const bool res = p.res != nullptr;
#ifndef DYOLO_L2E_BUILD
  if (p.bnb_mean) {  // training backward: z travels as the residual view, the sums as the forward statistics do
    static const int bw = dy_ablate("DYOLO_BNB_WGS") ? dy_ablate("DYOLO_BNB_WGS") : kBnbWgs;
    if (nch == 2 && bw == 2) {
      grid = hr_grid(2, nwork, p.tilesN);
      hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 2, false, false, true, 2>), dim3((unsigned)grid), dim3(256), 0, st, p);
    } else if (nch == 2) {
      hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 2, false, false, true, 3>), dim3((unsigned)grid), dim3(256), 0, st, p);
    } else {
      hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 4, false, false, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    }
    note_stats(grid / p.tilesN);
    return check_launch("conv3x3_hreg_kernel<bnb>");
  }
#endif
  if (p.stats) {  // (no residual here: dy_conv3x3_halo_route)
    if (nch == 1) hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 1, false, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else if (nch == 2) hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 2, false, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 4, false, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    note_stats(grid / p.tilesN);  // slots written: one per spatial block
    return check_launch("conv3x3_hreg_kernel");
  }
  if (nch == 1) {
    if (res) hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 1, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 1, false>), dim3((unsigned)grid), dim3(256), 0, st, p);
  } else if (nch == 2) {
    if (res) hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 2, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 2, false>), dim3((unsigned)grid), dim3(256), 0, st, p);
  } else {
    hipLaunchKernelGGL((conv3x3_hreg_kernel<T, 4, false>), dim3((unsigned)grid), dim3(256), 0, st, p);  // (no residual: dy_conv3x3_halo_route)
  }
  return check_launch("conv3x3_hreg_kernel");
}

template <typename T>
static int launch_hreg_s2(const HregArgs& a, hipStream_t st) {
  HregArgs p = a;
  const int grid = hr_grid(2, (long long)p.nSpatial * p.tilesN, p.tilesN);  // two 256-thread workgroups per CU (72 KB of LDS each)
#ifndef DYOLO_L2E_BUILD
  if (p.stats) {
    hipLaunchKernelGGL((conv3x3_hreg_s2_kernel<T, 2, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    note_stats(grid / p.tilesN);  // slots written: one per spatial block (at most 512 + 8 * tilesN - 1 workgroups)
    return check_launch("conv3x3_hreg_s2_kernel");
  }
#endif
  hipLaunchKernelGGL((conv3x3_hreg_s2_kernel<T, 2>), dim3((unsigned)grid), dim3(256), 0, st, p);
  return check_launch("conv3x3_hreg_s2_kernel");
}

// the fields both strides fill alike: pointers, dims, the geometry's tiles, byte sizes of the 16-bit views (dy_conv3x3_halo_route has checked them)
template <typename Geom>
static HregArgs hreg_args(const dy_conv_desc* d) {
  HregArgs a{};
  a.x = d->x, a.w = d->w, a.bias = d->bias, a.y = d->y;
  a.N = d->batch, a.H = d->h, a.W = d->w_in, a.Cin = d->cin, a.ldx = d->ld_x, a.Cout = d->cout, a.ldy = d->ld_y, a.act = d->act;
  a.tilesX = (d->wo + Geom::TW - 1) / Geom::TW;
  a.tilesY = (d->ho + Geom::TH - 1) / Geom::TH;
  a.tilesN = d->cout / 64;
  a.nSpatial = d->batch * a.tilesY * a.tilesX;
  a.x_bytes = (unsigned)((long long)d->batch * d->h * d->w_in * d->ld_x * 2), a.y_bytes = (unsigned)((long long)d->batch * d->ho * d->wo * d->ld_y * 2);
  return a;
}

// conv3x3_halo_dispatch's targets for the calls dy_conv3x3_halo_route (conv3x3_halo.hip) sends here: the route has checked the shape, the views'
// alignment and the ranges of 32-bit element offsets / buffer descriptors.
int conv3x3_hreg_s2_launch(const dy_conv_desc* d, hipStream_t st) {  // the 64-channel downsampling layers (conv3x3_hreg_s2_kernel)
  HregArgs a = hreg_args<HrS2>(d);
  a.stats = (d->y_dtype1 || d->bnb_z) ? nullptr : d->bn_stats;
  return d->dtype == DY_BF16 ? launch_hreg_s2<bf16_t>(a, st) : launch_hreg_s2<f16_t>(a, st);
}

int conv3x3_hreg_launch(const dy_conv_desc* d, hipStream_t st) {
  HregArgs a = hreg_args<HrS1>(d);
  a.stats = d->bn_stats;  // (at most 768 + 8 * tilesN - 1 workgroups: the slot count stays below the workspace's 1024)
  if (d->bnb_z) {
    const long long zb = (long long)d->batch * d->ho * d->wo * d->bnb_ld_z * 2;
#ifdef DYOLO_L2E_BUILD
    const bool built = false;  // (a gradient convolution carries no activation: it never comes through the scaled-domain build)
#else
    const bool built = d->bn_stats && !d->y_dtype1 && d->act == DY_ACT_NONE && d->cin != 32 && zb < (1ll << 32) - 64 && d->bnb_ld_z % 8 == 0 && (reinterpret_cast<uintptr_t>(d->bnb_z) & 15) == 0;
#endif
    if (built) {
      a.res = d->bnb_z, a.ldres = d->bnb_ld_z, a.r_bytes = (unsigned)zb;
      a.bnb_mean = d->bnb_mean, a.bnb_rstd = d->bnb_rstd, a.bnb_gamma = d->bnb_gamma, a.bnb_beta = d->bnb_beta, a.bnb_act = d->bnb_act;
    } else {
      a.stats = nullptr;  // (the caller's BatchNorm backward runs its own reduction: dy_conv_stats_written() stays 0)
    }
  }
  a.dbg = dy_ablate("DYOLO_DBG");
  return d->dtype == DY_BF16 ? launch_hreg<bf16_t>(a, st) : launch_hreg<f16_t>(a, st);
}

}  // namespace DY_NS
