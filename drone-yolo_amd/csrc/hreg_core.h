// The register-weight 3x3 family: what conv3x3_hreg.hip (stride 1 and 2), conv3x3_hhead.hip, conv3x3_hc2f.hip, conv3x3_hdown.hip and
// conv3x3_hsplit.hip share.  This comment is the family's description; each kernel file says only what it adds.
//
// Decomposition.  A wave owns ONE 16-cout MFMA fragment (hdown form A: two) and ALL pixels of the workgroup's output tile; its weights —
// 9 taps x NCH chunks of 32 channels x one A fragment = 36 / 72 / 144 VGPRs — are loaded once per workgroup lifetime (hr_load_wreg).
// Only the tile's halo patch of one 32-channel chunk lives in LDS, in a ring of stages, so two or three 256-thread workgroups fit a CU:
// independent waves per SIMD, each at its own point of its item, instead of two in barrier lock-step.  MFMA with the weight fragment as the
// A operand: a lane ends up with 4 consecutive couts of one pixel, from a bias-initialised accumulator summed chunk, halo row, kernel row,
// column (hr_rows_s1 / hr_rows_s2: 3 fragment reads per halo row feed up to 9 MFMAs, 0.42 ds_read_b128 per MFMA at stride 1).
//
// Image format.  A halo pixel's 32-channel chunk is 64 bytes (the pixel pitch) and its four 16-byte parts are stored with the part index
// XOR-ed with ((column key >> 1) & 3): every fragment read (16 pixels x 4 parts, any column shift) is bank-conflict free (4 LDS cycles, the
// minimum for ds_read_b128; an 80-byte pitch took 8) and all read addresses are `lane_base[q] + immediate`.  Two geometries:
//   HrS1  stride 1: 8 x 16 tile, 10 x 18 halo in rows of 24 slots (swizzle independent of the row), 16 KB stage, 4 LDS-DMA instructions per wave;
//   HrS2  stride 2: 4 x 16 tile, 9 x 33 halo kept as TWO column-parity planes per row (A: halo columns 0, 2, .., 32 at slot 0, B: columns
//         1, 3, .., 31 at slot 24; row pitch 40 slots = 2,560 B, both multiples of 256 B), so that the three taps of an output column are
//         unit-stride fragment reads again — A[j], B[j], A[j + 1]; 24 KB stage, 6 instructions per wave.
// The `mid` image of the fused kernels ([chunk][row][pixel 16] x 64 B, hr_mid_offset) has the same pixel format with the column as the key.
//
// Loader.  The image is lane-linear per wave-instruction (slot = (k * 4 + wave) * 16 + lane / 4, part = lane & 3), so it is filled by LDS-DMA
// with the swizzle applied to the SOURCE address: no staging registers, no ds_write pass.  The source is a BUFFER whose descriptor is shifted
// back by one image row + one pixel, so that every offset is non-negative: a lane's byte offset inside a tile's halo, rel[k] (hr_halo_rel), is a
// constant of the launch and the tile contributes a SCALAR offset (the instruction's soffset).  Interior tiles use rel[k] as it is; border
// tiles replace the out-of-image slots (hr_halo_inside) by an out-of-range offset, kHrOob, and the range check then feeds zeros: the zero
// padding.  No 64-bit address sums, no integer multiplies per slot and no zero-page selects (r03).  WHERE a kernel works out the border mask
// was chosen kernel by kernel against its register budget and stays there.
//
// Block order.  Persistent workgroups; blocks b and b + 8 share an XCD, so logical id = xcd * (G / 8) + b / 8 and an XCD's workgroups walk
// contiguous tiles: halo rows / columns shared by neighbours are L2 hits (hr_block; hr_grid makes G a multiple of 8 * tilesN).
//
// The drain rule.  Every item of every pipeline ends with the wave's FULL vector-memory drain (s_waitcnt vmcnt(0)) and then one barrier.
// Counted waits (vmcnt(4) / vmcnt(8): item i + 1 landed, item i + 2 left in flight) published a stage before all of its DMA had landed when
// another stream's kernels shared the CUs: the 64 -> 128 layers then read stale halo pixels, and results differed from run to run.  The
// full drain measured the same pass time.  The pipeline loops themselves (prologue, issue ahead, compute, drain + barrier, stage rotation)
// stay written out in each kernel: they differ in stage count and look-ahead, and they are where the hazards live.
//
// The store rule.  All of a tile's output stores leave back to back AFTER all of the epilogue's vector arithmetic, and nothing but the
// item's drain follows them (hr_store_tile).  First form of conv3x3_hc2f: fragment 0's stores, then fragment 1's SiLU.  The vector code behind
// a store re-used its data registers, and now and then — two workgroups per CU, several tiles per workgroup — the store sent the NEW content
// of one register in lanes 12..15 of every row of 16: a few wrong 4-byte pieces per thousand tiles, NaNs among them (always the last store
// in front of the arithmetic).  r09: conv3x3_hreg met the same thing with one fragment.  A build whose allocator rewrote the first data
// register of a 16-byte store in the very next instruction gave a BNB launch of 16 x 80 x 80 x 64 whose gradient differed from the plain launch's
// (the parent build left 2 to 11 instructions there, by luck).  Its stores stay among the epilogue's arithmetic (held back behind it they cost
// the 64-channel layers 1-2 %, 12.125 against 12.110 ms per pass) and hr_hold behind the item's drain keeps their data registers unwritten until
// they have retired.  Either way: no data register of an output store is written between the store and the drain.
#pragma once
#include "common_hip.h"

namespace DY_NS {

constexpr unsigned kHrOob = 0xfffffff0u;  // >= num_records of every 16-bit descriptor of the family (the hosts check the sizes)
constexpr int kHrVmcnt0 = 0x0f70;         // s_waitcnt vmcnt(0) alone (gfx9 encoding: expcnt 7 and lgkmcnt 15 = no wait)

// byte of part lq of the pixel in `slot` of an image row; `key` is the column the part swizzle goes by
__device__ __forceinline__ int hr_px(int slot, int key, int lq) { return slot * 64 + ((lq ^ ((key >> 1) & 3)) * 16); }

struct HrS1 {
  static constexpr int kStride = 1, TH = 8, TW = 16, HH = 10, HC = 18, kPitch = 24, kStage = 16 * 1024, NDMA = 4;  // 10 x 24 x 64 = 15,360 B, padded to 16 wave-instructions
  // the halo pixel (hy, hx) and swizzle key of the slot that lane `lane` of wave `wave` fills with its k-th instruction
  static __device__ __forceinline__ void slot(int k, int wave, int lane, int& hy, int& hx, int& key) {
    const int pix = ((k * 4 + wave) * 64 + lane) >> 2;
    hy = pix / kPitch, hx = pix - hy * kPitch, key = hx;
  }
  static __device__ __forceinline__ bool dead(int hy, int hx) { return hx >= HC || hy >= HH; }  // the row padding (hx >= 18) and the stage's padding (hy == 10): zeros for ever
  // fragment reads: pixel (row iy, column lr + q), part lq  ->  byte out[q] + iy * kPitch * 64
  static __device__ __forceinline__ void lane_base(int (&out)[3], int lr, int lq) {
#pragma unroll
    for (int q = 0; q < 3; ++q) out[q] = hr_px(lr + q, lr + q, lq);
  }
};

struct HrS2 {
  static constexpr int kStride = 2, TH = 4, TW = 16, HH = 9, HC = 33, kPitch = 40, kPlaneB = 24, kStage = 24 * 1024, NDMA = 6;  // 9 x 40 x 64 = 23,040 B, padded to 24 wave-instructions
  static __device__ __forceinline__ void slot(int k, int wave, int lane, int& hy, int& hx, int& key) {
    const int s = ((k * 4 + wave) * 64 + lane) >> 2;
    hy = s / kPitch;
    const int c = s - hy * kPitch;
    const bool planeB = c >= kPlaneB;
    key = planeB ? c - kPlaneB : c;         // column index inside the plane
    hx = planeB ? 2 * key + 1 : 2 * key;    // halo column
  }
  static __device__ __forceinline__ bool dead(int hy, int hx) { return hy >= HH || hx >= HC; }  // stage padding, plane padding
  // fragment reads of halo row iy: q = 0 -> plane A column lr, q = 1 -> plane B column lr, q = 2 -> plane A column lr + 1
  static __device__ __forceinline__ void lane_base(int (&out)[3], int lr, int lq) {
    out[0] = hr_px(lr, lr, lq);  // (also: pixel lr, part lq of a `mid` / operand row)
    out[1] = hr_px(kPlaneB + lr, lr, lq);
    out[2] = hr_px(lr + 1, lr + 1, lq);
  }
};

// ---- block order and tile decode ----
struct HrBlock { int nt, sb, Gs; };  // cout group, first spatial tile, spatial stride
__device__ __forceinline__ HrBlock hr_block(int G, int tilesN) {  // (tilesN == 1: the fused kernels)
  const int logical = ((int)blockIdx.x & 7) * (G >> 3) + ((int)blockIdx.x >> 3);
  return HrBlock{logical % tilesN, logical / tilesN, G / tilesN};
}
__device__ __forceinline__ int hr_my_tiles(int nSpatial, int sb, int Gs) { return sb < nSpatial ? (nSpatial - sb + Gs - 1) / Gs : 0; }

struct HrTile { int n, ty, tx; };
__device__ __forceinline__ HrTile hr_tile(int tile, int tilesX, int tilesY) {
  const int r = tile / tilesX;
  return HrTile{r / tilesY, r % tilesY, tile % tilesX};
}

// ---- this wave's weights: 16 couts (fragment `wave` of a 64-cout group at `base`) x all taps x NCH chunks, DY_WLAYOUT_HALO3X3 (NF = 4) ----
template <int NCH>
__device__ __forceinline__ void hr_load_wreg(u32x4 (&wreg)[NCH][9], const u32x4* base, int wave, int lane) {
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int t = 0; t < 9; ++t) wreg[c][t] = base[((c * 9 + t) * 4 + wave) * 64 + lane];
}

// ---- loader ----
// rel[k] = ((hy W + hx) ld) esz + part' pbytes: esz bytes per element, pbytes bytes per swizzled part (16-bit storage: 2, 16; split float16: 4, 32)
template <typename Geom>
__device__ __forceinline__ void hr_halo_rel(unsigned (&rel)[Geom::NDMA], int wave, int lane, int W, int ld, unsigned esz, unsigned pbytes, unsigned oob = kHrOob) {
#pragma unroll
  for (int k = 0; k < Geom::NDMA; ++k) {
    int hy, hx, key;
    Geom::slot(k, wave, lane, hy, hx, key);
    rel[k] = Geom::dead(hy, hx) ? oob : (unsigned)((hy * W + hx) * ld) * esz + (unsigned)((lane & 3) ^ ((key >> 1) & 3)) * pbytes;
  }
}
// (y0, x0): input coordinates of the centre tap of the tile's first output pixel.  No slot of the halo is outside the image (wave-uniform):
template <typename Geom>
__device__ __forceinline__ bool hr_interior(int y0, int x0, int H, int W) { return y0 > 0 && y0 - 1 + Geom::HH <= H && x0 > 0 && x0 - 1 + Geom::HC <= W; }
// the border test of one slot
template <typename Geom>
__device__ __forceinline__ bool hr_halo_inside(int k, int wave, int lane, int y0, int x0, int H, int W) {
  int hy, hx, key;
  Geom::slot(k, wave, lane, hy, hx, key);
  return (unsigned)(y0 - 1 + hy) < (unsigned)H && (unsigned)(x0 - 1 + hx) < (unsigned)W;
}
// the wave's k-th LDS-DMA instruction of an image at `sa`: 64 lanes x 16 bytes into block k * 4 + wave
__device__ __forceinline__ void hr_issue1(__amdgpu_buffer_rsrc_t rs, unsigned char* sa, int k, int wave, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(sa + (k * 4 + wave) * 1024), 16, (int)voff, (int)soff, 0, 0);
}
template <int NDMA>
__device__ __forceinline__ void hr_issue(__amdgpu_buffer_rsrc_t rs, unsigned char* sa, int wave, const unsigned (&voff)[NDMA], unsigned soff) {
#pragma unroll
  for (int k = 0; k < NDMA; ++k) hr_issue1(rs, sa, k, wave, voff[k], soff);
}

// ---- compute: one chunk of one tile.  dbg (-DDYOLO_ABLATE builds only, else a constant 0): 2 no MFMAs, 8 no fragment reads ----
template <typename T, int NCH>
__device__ __forceinline__ void hr_rows_s1(f32x4 (&acc)[HrS1::TH], const u32x4 (&wreg)[NCH][9], const unsigned char* sa, const int (&lane_base)[3], int c, int dbg = 0) {
#pragma unroll
  for (int iy = 0; iy < HrS1::HH; ++iy) {
    u32x4 a[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] = *reinterpret_cast<const u32x4*>(sa + lane_base[q] + ((dbg & 8) ? 0 : iy * (HrS1::kPitch * 64)));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int o = iy - r;
      if (o >= 0 && o < HrS1::TH) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if (dbg & 2) asm volatile("" ::"v"(a[q]));
          else acc[o] = Elem<T>::mma(wreg[c][r * 3 + q], a[q], acc[o]);  // D[cout][pixel]
        }
      }
    }
  }
}
// stride 2: even halo rows feed the kernel rows r = 0 and r = 2 of two output rows (6 MFMAs per 3 reads and fragment), odd rows r = 1 (3 per 3)
template <typename T, int NF3, int NCH>
__device__ __forceinline__ void hr_rows_s2(f32x4 (&acc)[NF3][HrS2::TH], const u32x4 (&wreg)[NF3][NCH][9], const unsigned char* sa, const int (&lane_base)[3], int c) {
#pragma unroll
  for (int iy = 0; iy < HrS2::HH; ++iy) {
    u32x4 a[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] = *reinterpret_cast<const u32x4*>(sa + lane_base[q] + iy * (HrS2::kPitch * 64));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      if ((iy - r) % 2 == 0) {
        const int o = (iy - r) / 2;
        if (iy - r >= 0 && o < HrS2::TH) {
#pragma unroll
          for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int f = 0; f < NF3; ++f) acc[f][o] = Elem<T>::mma(wreg[f][c][r * 3 + q], a[q], acc[f][o]);  // D[cout][pixel]
        }
      }
    }
  }
}

// ---- epilogue ----
// A result lane holds 8 bytes (4 channels) of pixel lr in tile row o.  Stored like that, each of the 64 lanes is its own L1 request.
// v_permlane16_swap between the rows of a pair (o, o + 1) leaves 16 contiguous bytes in every lane - quarter lq gets channels
// 8 (lq >> 1) .. + 7 of row o + (lq & 1) - so a pair of rows leaves in one 16-byte store instead of two 8-byte ones.
__device__ __forceinline__ u32x4 hr_pack_pair(u32x2 pk_o, u32x2 pk_o1) {
  const auto sx = __builtin_amdgcn_permlane16_swap(pk_o[0], pk_o1[0], false, false);
  const auto sy = __builtin_amdgcn_permlane16_swap(pk_o[1], pk_o1[1], false, false);
  return u32x4{sx[0], sy[0], sx[1], sy[1]};
}
// the swap run backwards: a row pair's 16-byte piece (loaded in store order) back in result-lane order, row `odd` of the pair
__device__ __forceinline__ u32x2 hr_unpack_pair(u32x4 piece, int odd) {
  const auto sx = __builtin_amdgcn_permlane16_swap(piece[0], piece[2], false, false);
  const auto sy = __builtin_amdgcn_permlane16_swap(piece[1], piece[3], false, false);
  return u32x2{sx[odd], sy[odd]};
}
// the lane's part of a store offset: row o + (lq & 1) of pair o / 2, column lr, channel co8 (the lane's 8-channel group)
template <int TH>
__device__ __forceinline__ void hr_lane_out(unsigned (&lane_out)[TH / 2], int lr, int lq, int Wo, int ldy, int co8, unsigned esz) {
#pragma unroll
  for (int o = 0; o < TH; o += 2) lane_out[o / 2] = (unsigned)(((o + (lq & 1)) * Wo + lr) * ldy + co8) * esz;
}
// hand-over of a fused kernel: a result lane of the 3x3 holds channels wave * 16 + lq * 4 .. + 3 of pixel (o, lr), 8 bytes of `mid` / of an
// operand image at hr_mid_offset + o * 1024 (chunk_bytes: one 32-channel chunk of the tile)
__device__ __forceinline__ int hr_mid_offset(int wave, int lr, int lq, int chunk_bytes) {
  return (wave >> 1) * chunk_bytes + hr_px(lr, lr, (wave & 1) * 2 + (lq >> 1)) + (lq & 1) * 8;
}
// the 3x3's epilogue of a fused kernel: SiLU (+ the residual from its operand image `res`), ONE rounding to the storage type (where the
// layer-by-layer path rounds), into `mid`; both pointers already carry hr_mid_offset
template <typename T, int TH, bool RES>
__device__ __forceinline__ void hr_tail_mid(const f32x4 (&acc)[TH], unsigned char* mid, const unsigned char* res) {
  typedef __attribute__((ext_vector_type(4))) T t4;
#pragma unroll
  for (int o = 0; o < TH; ++o) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = silu_f32(acc[o][e]);
    if constexpr (RES) {
      const t4 rr = __builtin_bit_cast(t4, *reinterpret_cast<const u32x2*>(res + o * 1024));
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += Elem<T>::to_f32(rr[e]);
    }
    t4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = Elem<T>::from_f32(v[e]);
    *reinterpret_cast<u32x2*>(mid + o * 1024) = __builtin_bit_cast(u32x2, ov);
  }
}
// in front of an epilogue that reads fresh accumulators: the tile's last MFMAs have retired before the vector code reads them, whatever
// the scheduler does around here
__device__ __forceinline__ void hr_settle_mfma() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
// The store rule (header): NFRAG x NPAIR 16-byte stores per lane, back to back.  The empty asm statements pin every operand of the stores in
// front of them: no arithmetic is scheduled or sunk between the stores.
template <int NFRAG, int NPAIR>
__device__ __forceinline__ void hr_store_tile(u32x4 (&st)[NFRAG][NPAIR], unsigned (&off)[NPAIR], __amdgpu_buffer_rsrc_t rs, unsigned out_base, unsigned frag_stride) {
#pragma unroll
  for (int f = 0; f < NFRAG; ++f)
#pragma unroll
    for (int h = 0; h < NPAIR; ++h) asm volatile("" : "+v"(st[f][h]));
#pragma unroll
  for (int h = 0; h < NPAIR; ++h) asm volatile("" : "+v"(off[h]));
#pragma unroll
  for (int f = 0; f < NFRAG; ++f)
#pragma unroll
    for (int h = 0; h < NPAIR; ++h) __builtin_amdgcn_raw_buffer_store_b128(st[f][h], rs, off[h], (int)(out_base + (unsigned)f * frag_stride), 0);
}
// the store rule's other form (conv3x3_hreg): placed BEHIND the drain that retires the stores of `st`, it keeps their data registers live
// (unwritten) until then
template <int N>
__device__ __forceinline__ void hr_hold(const u32x4 (&st)[N]) {
#pragma unroll
  for (int h = 0; h < N; ++h) asm volatile("" ::"v"(st[h]));
}
// the closing 1x1's epilogue of hc2f / hdown: bias last (as conv1x1_stream adds it), SiLU, the wave's two fragments of the tile at output
// coordinates (y0, x0) of an Ho x Wo map, then hr_store_tile
template <typename T, int TH>
__device__ __forceinline__ void hr_out_1x1(const f32x4 (&acc1)[2][TH], const f32x4 (&bias1)[2], const unsigned (&lane_out)[TH / 2], __amdgpu_buffer_rsrc_t rs, unsigned out_base,
                                           int y0, int x0, int Ho, int Wo, int lr, int lq) {
  typedef __attribute__((ext_vector_type(4))) T t4;
  const bool whole = y0 + TH <= Ho && x0 + 16 <= Wo;  // wave-uniform: no ragged edge
  u32x4 st[2][TH / 2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    u32x2 pk[TH];
#pragma unroll
    for (int o = 0; o < TH; ++o) {
      t4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = Elem<T>::from_f32(silu_f32(acc1[f][o][e] + bias1[f][e]));
      pk[o] = __builtin_bit_cast(u32x2, ov);
    }
#pragma unroll
    for (int o = 0; o < TH; o += 2) st[f][o / 2] = hr_pack_pair(pk[o], pk[o + 1]);
  }
  unsigned off[TH / 2];
#pragma unroll
  for (int o = 0; o < TH; o += 2) {
    off[o / 2] = lane_out[o / 2];
    if (!whole) off[o / 2] = (y0 + o + (lq & 1) < Ho && x0 + lr < Wo) ? off[o / 2] : kHrOob;
  }
  hr_store_tile<2, TH / 2>(st, off, rs, out_base, 16u * (unsigned)sizeof(T));
}

// ---- statistics slots of a dy_bn_train_fwd workspace: spatial block sb owns slot 1 + sb, slot 0 holds the totals ----
__device__ __forceinline__ void hr_stats_zero(double* stats, int Cout, int nt, int sb, int tid, bool has_tiles) {
  if (blockIdx.x == 0)  // the totals the BatchNorm's partial-sum launch adds into
    for (int i = tid; i < 2 * Cout; i += 256) stats[i] = 0.0;
  if (!has_tiles && tid < 128) {  // a slot is summed whether its workgroup had tiles or not
    const int co = nt * 64 + (tid & 63);
    if (co < Cout) stats[(size_t)(1 + sb) * 2 * Cout + (tid >> 6) * Cout + co] = 0.0;
  }
}
// one shuffle reduction over the 16 pixel lanes of a quarter, 32 plain stores per wave
__device__ __forceinline__ void hr_stats_store(double* stats, int Cout, int nt, int sb, int wave, int lq, int lr, const float (&st_sum)[4], const float (&st_sq)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a = st_sum[e], b = st_sq[e];
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) a += __shfl_xor(a, m, 64), b += __shfl_xor(b, m, 64);
    const int co = nt * 64 + wave * 16 + lq * 4 + e;
    if (lr == 0 && co < Cout) {
      double* slot = stats + (size_t)(1 + sb) * 2 * Cout;
      slot[co] = (double)a, slot[Cout + co] = (double)b;
    }
  }
}

// ---- host: persistent grid of wgs_per_cu workgroups on each of the 256 CUs, clamped to the work; the XCD order and the fixed cout group
// per block need G % (8 * tilesN) == 0 ----
static inline int hr_grid(int wgs_per_cu, long long nwork, int tilesN) {
  int grid = 256 * wgs_per_cu;
  if (nwork < grid) grid = (int)nwork;
  const int q = 8 * tilesN;
  return (grid + q - 1) / q * q;
}

}  // namespace DY_NS
