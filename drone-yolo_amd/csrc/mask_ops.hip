// Instance segmentation on the device (include/dyolo.h): the depth-to-space half of Proto's ConvTranspose2d(c, c, 2, 2), the gather of
// the kept detections' mask coefficients behind dy_nms, and the mask assembly of a whole batch (ops.process_mask / process_mask_native
// of the reference, utils/ops.py:660-753) in one launch.
#include "common_hip.h"
#include "mask_crop.h"
#include "tile_limits.h"

namespace dy {

static inline int mask_grid_for(long long total, int per_block = 256) {
  long long g = (total + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > 65536) g = 65536;
  return (int)g;
}

// ---- dy_depth_to_space2_nhwc: one 16-byte chunk per thread (grid-stride); cp = chunks per OUTPUT pixel --------------------------------
__global__ __launch_bounds__(256) void depth_to_space2_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int n, int ho, int wo, int cp,
                                                              int lds_c, int ldd_c) {
  const long long total = (long long)n * ho * wo * cp;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % cp);
    long long p = i / cp;
    const int ox = (int)(p % wo);
    p /= wo;
    const int oy = (int)(p % ho);
    const long long b = p / ho;
    const int q = ((oy & 1) << 1) | (ox & 1);
    const long long sp = (b * (ho >> 1) + (oy >> 1)) * (wo >> 1) + (ox >> 1);
    dst[((b * ho + oy) * wo + ox) * ldd_c + k] = src[sp * lds_c + q * cp + k];
  }
}

// ---- dy_mask_gather: one thread per (image, row, column of the side buffer) -----------------------------------------------------------
struct GatherArgs {
  const float* rows;
  const int* counts;
  const int* index;
  const float* level[DY_MAX_LEVELS];
  int hw[DY_MAX_LEVELS], ld[DY_MAX_LEVELS], a0[DY_MAX_LEVELS + 1];
  int n_levels;
  const float* pred;
  int pred_ch, pred_c0, anchors, batch, max_det, nm;
  float* out;
};

__global__ __launch_bounds__(256) void mask_gather_kernel(GatherArgs a) {
  const int cols = 4 + a.nm;
  const long long total = (long long)a.batch * a.max_det * cols;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int j = (int)(i % cols);
    const long long br = i / cols;
    const int r = (int)(br % a.max_det), b = (int)(br / a.max_det);
    if (r >= a.counts[b]) continue;  // rows beyond the count: neither read nor written
    float v = 0.f;
    if (j < 4) {
      v = a.rows[br * 6 + j];
    } else {
      const int k = j - 4, an = a.index[br];
      if (an >= 0 && an < a.anchors) {
        if (a.pred) {
          v = a.pred[((long long)b * a.pred_ch + a.pred_c0 + k) * a.anchors + an];
        } else {
          for (int l = 0; l < a.n_levels; ++l)
            if (an >= a.a0[l] && an < a.a0[l + 1]) v = a.level[l][((long long)b * a.hw[l] + (an - a.a0[l])) * a.ld[l] + k];
        }
      }
    }
    a.out[i] = v;
  }
}

// ---- dy_process_mask -------------------------------------------------------------------------------------------------------------------
// One workgroup = one detection x one run of kPixPerBlock output pixels of its (oh, ow) mask.  The mask is a run of oh * ow bytes at
// t * oh * ow of the output; a thread owns 8 consecutive, 8-byte aligned bytes of it (one 64-bit store); the at most 7 bytes in front of
// the first and behind the last aligned group of a mask are written one by one by the workgroup that owns the neighbouring group.  The 32
// coefficients are workgroup-uniform (registers); a corner is one 128-byte proto row (8 x 16-byte loads of one lane) and a 32-term fp32
// dot product.  Consecutive output pixels share corner columns (ratio 4: four pixels per source pixel), so a thread keeps the two columns
// of its last pixel and recomputes one only when the source column moves.  Pixels outside the detection's bounding region (the crop window
// mapped to the output, plus one source pixel) cost a compare; whole groups outside it are stored as zeros.
constexpr int kPmThreads = 256, kPmGroups = 4, kPixPerBlock = kPmThreads * 8 * kPmGroups;

struct PmArgs {
  const float* protos;
  const float* side;
  const int* counts;
  const int* offsets;
  const int* window;
  const float* crop_rows;
  int batch, max_det, mh, mw, ld_p, oh, ow, total, crop_at_output;
  float ratio_x, ratio_y;
  FastDiv div_ow;  // a pixel's offset inside its mask is below oh * ow < 2^31 (the host checks the launch grid): exact 32-bit division by ow
  unsigned char* out;
};

struct PmDet {  // workgroup-uniform state of one detection
  const float* proto;  // the image's grid at the window's origin
  int sh, sw, ld_p, mw_ld;  // mw_ld: elements per proto row
  float scale_y, scale_x;
  int cx_lo, cx_hi, cy_lo, cy_hi;  // crop at proto resolution (window coordinates), inclusive; crop_at_output: the whole window
  int rx_lo, rx_hi, ry_lo, ry_hi;  // bounding region in output pixels, inclusive (empty when lo > hi)
  float bx1, by1, bx2, by2;        // crop_at_output: the box in output pixels
  int crop_out;
  float cf[32];
};

__device__ __forceinline__ float pm_dot(const PmDet& D, int yy, int xx) {
  return proto_dot32(D.cf, D.proto + (long long)yy * D.mw_ld + (long long)xx * D.ld_p);
}

struct PmCol {  // the two corner values (rows y0, y1) of one source column
  int x;
  float top, bot;
};

__device__ __forceinline__ PmCol pm_column(const PmDet& D, int xx, int y0, int y1) {
  PmCol c;
  c.x = xx;
  const bool xin = xx >= D.cx_lo && xx <= D.cx_hi;
  c.top = (xin && y0 >= D.cy_lo && y0 <= D.cy_hi) ? pm_dot(D, y0, xx) : 0.f;
  c.bot = (y1 == y0) ? c.top : ((xin && y1 >= D.cy_lo && y1 <= D.cy_hi) ? pm_dot(D, y1, xx) : 0.f);
  return c;
}

__device__ __forceinline__ float pm_src(float scale, int dst) { return pm_src_at(scale, (float)dst + 0.5f); }

// 0 / 1 of output pixel (y, x); (A, B, cy) carry the columns of the thread's previous pixel (cy: the row they belong to, -1: none)
__device__ __forceinline__ unsigned pm_pixel(const PmDet& D, int y, int x, PmCol& A, PmCol& B, int& cy) {
  if (y < D.ry_lo || y > D.ry_hi || x < D.rx_lo || x > D.rx_hi) return 0u;
  if (D.crop_out) {
    const float fx = (float)x, fy = (float)y;
    if (!(fx >= D.bx1 && fx < D.bx2 && fy >= D.by1 && fy < D.by2)) return 0u;
  }
  const float sy = pm_src(D.scale_y, y), sx = pm_src(D.scale_x, x);
  int y0 = (int)sy, x0 = (int)sx;
  y0 = y0 > D.sh - 1 ? D.sh - 1 : y0;
  x0 = x0 > D.sw - 1 ? D.sw - 1 : x0;
  const int y1 = y0 + (y0 < D.sh - 1 ? 1 : 0), x1 = x0 + (x0 < D.sw - 1 ? 1 : 0);
  const float ly1 = sy - (float)y0, lx1 = sx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  if (cy != y) {
    A.x = B.x = -1;
    cy = y;
  }
  if (A.x != x0) A = (B.x == x0) ? B : pm_column(D, x0, y0, y1);
  if (B.x != x1) B = (A.x == x1) ? A : pm_column(D, x1, y0, y1);
  const float v = pm_blend(ly0, ly1, lx0, lx1, A.top, B.top, A.bot, B.bot);
  return v > 0.f ? 1u : 0u;
}

__global__ __launch_bounds__(kPmThreads) void process_mask_kernel(PmArgs a) {
  const int t = blockIdx.x;
  const long long P = (long long)a.oh * a.ow;
  const long long start = (long long)t * P, end = start + P;  // this mask's bytes
  // which image / row (offsets is an exclusive prefix of counts; anything inconsistent gives a zero mask)
  int b = -1;
  for (int i = 0; i < a.batch; ++i)
    if (t >= a.offsets[i] && t < a.offsets[i + 1]) b = i;
  int r = b >= 0 ? t - a.offsets[b] : 0;
  const bool live = b >= 0 && r >= 0 && r < a.max_det && r < a.counts[b];

  PmDet D;
  D.rx_lo = D.ry_lo = 0;
  D.rx_hi = D.ry_hi = -1;
  D.crop_out = a.crop_at_output;
  D.ld_p = a.ld_p;
  D.mw_ld = a.mw * a.ld_p;
  D.sh = D.sw = 1;
  D.scale_x = D.scale_y = 1.f;
  D.cx_lo = D.cy_lo = 0;
  D.cx_hi = D.cy_hi = -1;
  D.bx1 = D.by1 = D.bx2 = D.by2 = 0.f;
  D.proto = a.protos;
#pragma unroll
  for (int k = 0; k < 32; ++k) D.cf[k] = 0.f;
  if (live) {
    const float* srow = a.side + ((long long)b * a.max_det + r) * 36;
#pragma unroll
    for (int k = 0; k < 32; ++k) D.cf[k] = srow[4 + k];
    int top = a.window[4 * b + 0], left = a.window[4 * b + 1], sh = a.window[4 * b + 2], sw = a.window[4 * b + 3];
    top = min(max(top, 0), a.mh - 1);
    left = min(max(left, 0), a.mw - 1);
    sh = min(max(sh, 1), a.mh - top);
    sw = min(max(sw, 1), a.mw - left);
    D.sh = sh;
    D.sw = sw;
    D.proto = a.protos + ((long long)b * a.mh + top) * D.mw_ld + (long long)left * a.ld_p;
    D.scale_y = (float)sh / (float)a.oh;
    D.scale_x = (float)sw / (float)a.ow;
    if (a.crop_at_output) {
      const float* cr = a.crop_rows + ((long long)b * a.max_det + r) * 6;
      D.bx1 = cr[0], D.by1 = cr[1], D.bx2 = cr[2], D.by2 = cr[3];
      D.cx_lo = 0, D.cx_hi = sw - 1, D.cy_lo = 0, D.cy_hi = sh - 1;
      // pixels with bx1 <= x < bx2 (clamped through float so that huge boxes cannot overflow the int conversion)
      D.rx_lo = (int)ceilf(fminf(fmaxf(D.bx1, 0.f), (float)a.ow));
      D.rx_hi = (int)ceilf(fminf(fmaxf(D.bx2, 0.f), (float)a.ow)) - 1;
      D.ry_lo = (int)ceilf(fminf(fmaxf(D.by1, 0.f), (float)a.oh));
      D.ry_hi = (int)ceilf(fminf(fmaxf(D.by2, 0.f), (float)a.oh)) - 1;
    } else {
      // crop_mask at proto resolution: xx >= bx1 and xx < bx2 (window == whole grid in this mode, offsets taken out all the same)
      const float x1 = srow[0] * a.ratio_x - (float)left, x2 = srow[2] * a.ratio_x - (float)left;
      const float y1 = srow[1] * a.ratio_y - (float)top, y2 = srow[3] * a.ratio_y - (float)top;
      const CropWin cw = crop_window(x1, y1, x2, y2, sw, sh);  // (mask_crop.h: the NaN-corner rule lives there)
      D.cx_lo = cw.x_lo, D.cx_hi = cw.x_hi, D.cy_lo = cw.y_lo, D.cy_hi = cw.y_hi;
      if (D.cx_lo <= D.cx_hi && D.cy_lo <= D.cy_hi) {
        // output pixels whose corners can touch the crop: source coordinate in (c_lo - 1, c_hi + 1), one output pixel of slack each side
        const float ix = (float)a.ow / (float)sw, iy = (float)a.oh / (float)sh;
        D.rx_lo = max((int)floorf(((float)D.cx_lo - 0.5f) * ix - 0.5f) - 1, 0);
        D.rx_hi = min((int)ceilf(((float)D.cx_hi + 1.5f) * ix - 0.5f) + 1, a.ow - 1);
        D.ry_lo = max((int)floorf(((float)D.cy_lo - 0.5f) * iy - 0.5f) - 1, 0);
        D.ry_hi = min((int)ceilf(((float)D.cy_hi + 1.5f) * iy - 0.5f) + 1, a.oh - 1);
      }
    }
  }

  const long long a0 = (start + 7) & ~7ll, a1 = end & ~7ll;  // aligned groups [a0, a1) lie wholly inside this mask
  const long long run0 = a0 + (long long)blockIdx.y * kPixPerBlock;
  PmCol A, B;
  A.x = B.x = -1;
  A.top = A.bot = B.top = B.bot = 0.f;
  int cy = -1;
  if (a1 > a0) {
#pragma unroll 1
    for (int g = 0; g < kPmGroups; ++g) {
      const long long g0 = run0 + ((long long)g * kPmThreads + threadIdx.x) * 8;
      if (g0 >= a1) break;
      const unsigned p = (unsigned)(g0 - start);
      int y = (int)fastdiv(p, a.div_ow), x = (int)(p - (unsigned)y * (unsigned)a.ow);
      unsigned long long word = 0ull;
      const bool row_dead = y < D.ry_lo || y > D.ry_hi, same_row = x + 7 < a.ow;
      if (!(same_row && (row_dead || x > D.rx_hi || x + 7 < D.rx_lo))) {
#pragma unroll 1
        for (int e = 0; e < 8; ++e) {
          word |= (unsigned long long)pm_pixel(D, y, x, A, B, cy) << (8 * e);
          if (++x == a.ow) x = 0, ++y;
        }
      }
      *reinterpret_cast<unsigned long long*>(a.out + g0) = word;
    }
  }
  // the bytes in front of the first / behind the last aligned group (at most 7 each; all of a mask that holds no aligned group: < 15)
  if (blockIdx.y == 0) {
    const long long head_end = a1 > a0 ? a0 : end;
    const long long i = start + threadIdx.x;
    if (threadIdx.x < 16 && i < head_end) {
      const unsigned p = (unsigned)(i - start);
      const int y = (int)fastdiv(p, a.div_ow), x = (int)(p - (unsigned)y * (unsigned)a.ow);
      cy = -1;
      a.out[i] = (unsigned char)pm_pixel(D, y, x, A, B, cy);
    }
    const long long j = a1 + ((int)threadIdx.x - 16);
    if (a1 > a0 && threadIdx.x >= 16 && threadIdx.x < 24 && j < end) {
      const unsigned p = (unsigned)(j - start);
      const int y = (int)fastdiv(p, a.div_ow), x = (int)(p - (unsigned)y * (unsigned)a.ow);
      cy = -1;
      a.out[j] = (unsigned char)pm_pixel(D, y, x, A, B, cy);
    }
  }
}

// ---- dy_tile_process_mask ----------------------------------------------------------------------------------------------------
// Frame masks of tiled inference, driven by candidate: blockIdx.x = slot j = k * max_det + r of frame blockIdx.z.  A slot below its tile's
// count whose owner t is a kept row with dest[t] = m >= 0 ORs its tile's mask into mask m of the output; every other workgroup leaves at
// once and reads nothing more.  The workgroups of a live slot (gridDim.y of them, striding) cover the bounding region of its crop window in
// output pixels, one aligned 32-bit word of the output (four bytes of one mask row) per thread: the four pixels share corner columns as in
// dy_process_mask, and a word that holds a set pixel is OR-ed in with one integer atomic, so members of one row in overlapping tiles meet
// in any order with the same result.  The entry point zeroes the output in front (tile_mask_zero_kernel on the same stream).  The pixel itself is
// dy_process_mask's: pm_src_at / pm_column / pm_blend on the tile's proto grid at scale 0.25, the output pixel's centre taken in tile pixels.
constexpr int kTpmThreads = 256;

struct TpmArgs {
  const float* protos;
  const float* side;
  const int* counts;
  const int* offs;
  const int* owner;
  const int* dest;
  unsigned char* out;
  int K, max_det, N, keep, mh, mw, ld_p, th, tw, oh, ow, s, total;
};

// Zeroes `bytes` bytes at the 4-byte aligned p: 16-byte stores where p allows them, then the words and the at most three bytes that are left.
// (A kernel, not a memset: see zero_async in common_hip.h.)
__global__ __launch_bounds__(256) void tile_mask_zero_kernel(unsigned char* p, long long bytes, int vec) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
  const long long n16 = vec ? bytes / 16 : 0;
  for (long long i = gid; i < n16; i += step) reinterpret_cast<u32x4*>(p)[i] = u32x4{0u, 0u, 0u, 0u};
  const long long n4 = bytes / 4;
  for (long long i = n16 * 4 + gid; i < n4; i += step) reinterpret_cast<unsigned*>(p)[i] = 0u;
  for (long long i = n4 * 4 + gid; i < bytes; i += step) p[i] = 0;
}

__global__ __launch_bounds__(kTpmThreads) void tile_process_mask_kernel(TpmArgs a) {
  const int f = blockIdx.z, j = blockIdx.x;
  const int tile = j / a.max_det, r = j - tile * a.max_det;
  const long long b = (long long)f * a.K + tile;
  if (r >= a.counts[b]) return;
  const int t = a.owner[(long long)f * a.N + j];
  if (t < 0 || t >= a.keep) return;
  const int m = a.dest[(long long)f * a.keep + t];
  if (m < 0 || m >= a.total) return;

  const float* srow = a.side + (b * a.max_det + r) * 36;
  const CropWin cw = crop_window(srow[0] * 0.25f, srow[1] * 0.25f, srow[2] * 0.25f, srow[3] * 0.25f, a.mw, a.mh);
  if (cw.x_lo > cw.x_hi || cw.y_lo > cw.y_hi) return;
  PmDet D;
  D.ld_p = a.ld_p;
  D.mw_ld = a.mw * a.ld_p;
  D.sh = a.mh, D.sw = a.mw;
  D.proto = a.protos + b * a.mh * D.mw_ld;
  D.cx_lo = cw.x_lo, D.cx_hi = cw.x_hi, D.cy_lo = cw.y_lo, D.cy_hi = cw.y_hi;
#pragma unroll
  for (int k = 0; k < 32; ++k) D.cf[k] = srow[4 + k];

  // Tile pixels whose corners can touch the crop: source coordinate in [c_lo - 1, c_hi + 1), i.e. t in [4 c_lo - 2, 4 c_hi + 6); then the
  // output pixels whose centres (X + 0.5) * s - o can lie there, one pixel of slack each side (the pixel test below is the exact one).
  const int oy = a.offs[2 * tile], ox = a.offs[2 * tile + 1];
  const float fs = (float)a.s, inv = 1.f / fs;
  const int tx_lo = max(4 * cw.x_lo - 2, 0), tx_hi = min(4 * cw.x_hi + 6, a.tw - 1);
  const int ty_lo = max(4 * cw.y_lo - 2, 0), ty_hi = min(4 * cw.y_hi + 6, a.th - 1);
  const int X_lo = max((int)floorf((float)(tx_lo + ox) * inv) - 1, 0), X_hi = min((int)floorf((float)(tx_hi + ox) * inv) + 1, a.ow - 1);
  const int Y_lo = max((int)floorf((float)(ty_lo + oy) * inv) - 1, 0), Y_hi = min((int)floorf((float)(ty_hi + oy) * inv) + 1, a.oh - 1);
  if (X_lo > X_hi || Y_lo > Y_hi) return;
  const int W = X_hi - X_lo + 1, H = Y_hi - Y_lo + 1;
  const int wpr = (W + 3) / 4 + 1;  // aligned words that can hold a row's W bytes
  const long long items = (long long)H * wpr;
  const long long base = (long long)m * a.oh * a.ow, bytes = (long long)a.total * a.oh * a.ow;
  const float foy = (float)oy, fox = (float)ox, fth = (float)a.th, ftw = (float)a.tw;

  for (long long i = (long long)blockIdx.y * kTpmThreads + threadIdx.x; i < items; i += (long long)gridDim.y * kTpmThreads) {
    const int row = (int)(i / wpr), wi = (int)(i - (long long)row * wpr);
    const int Y = Y_lo + row;
    const long long rowbase = base + (long long)Y * a.ow;
    const long long g_lo = rowbase + X_lo, g_hi = rowbase + X_hi;
    const long long w0 = ((g_lo >> 2) + wi) << 2;  // first byte of this thread's word
    if (w0 > g_hi) continue;
    const float ty = ((float)Y + 0.5f) * fs - foy;
    if (!(ty >= 0.f && ty < fth)) continue;
    const float sy = pm_src_at(0.25f, ty);
    int y0 = (int)sy;
    y0 = y0 > a.mh - 1 ? a.mh - 1 : y0;
    const int y1 = y0 + (y0 < a.mh - 1 ? 1 : 0);
    const float ly1 = sy - (float)y0, ly0 = 1.f - ly1;
    PmCol A, B;
    A.x = B.x = -1;
    A.top = A.bot = B.top = B.bot = 0.f;
    unsigned word = 0u;
#pragma unroll 1
    for (int e = 0; e < 4; ++e) {
      const long long g = w0 + e;
      if (g < g_lo || g > g_hi) continue;
      const int X = (int)(g - rowbase);
      const float tx = ((float)X + 0.5f) * fs - fox;
      if (!(tx >= 0.f && tx < ftw)) continue;
      const float sx = pm_src_at(0.25f, tx);
      int x0 = (int)sx;
      x0 = x0 > a.mw - 1 ? a.mw - 1 : x0;
      const int x1 = x0 + (x0 < a.mw - 1 ? 1 : 0);
      const float lx1 = sx - (float)x0, lx0 = 1.f - lx1;
      if (A.x != x0) A = (B.x == x0) ? B : pm_column(D, x0, y0, y1);
      if (B.x != x1) B = (A.x == x1) ? A : pm_column(D, x1, y0, y1);
      const float v = pm_blend(ly0, ly1, lx0, lx1, A.top, B.top, A.bot, B.bot);
      if (v > 0.f) word |= 1u << (8 * e);
    }
    if (word == 0u) continue;
    if (w0 + 4 <= bytes) {
      atomicOr(reinterpret_cast<unsigned*>(a.out + w0), word);
    } else {  // the buffer's last, partial word: every writer of it stores bytes
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((word >> (8 * e)) & 1u) a.out[w0 + e] = 1;
    }
  }
}

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_depth_to_space2_nhwc(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_src, int32_t ld_dst,
                                           int32_t dtype, dy_stream_t stream) {
  const int es = dtype == DY_FP8 ? 0 : dy_dtype_size(dtype);
  DY_REQUIRE(src && dst && es, DY_ERR_INVALID_ARG, "dy_depth_to_space2_nhwc: null pointer or bad dtype");
  DY_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, DY_ERR_INVALID_ARG, "dy_depth_to_space2_nhwc: bad dims");
  DY_REQUIRE(c % 8 == 0, DY_ERR_UNSUPPORTED, "dy_depth_to_space2_nhwc: c must be a multiple of 8 (whole 16-byte chunks in every storage type)");
  const int epc = 16 / es;
  DY_REQUIRE(ld_src >= 4 * c && ld_dst >= c && ld_src % epc == 0 && ld_dst % epc == 0 && aligned16(src) && aligned16(dst), DY_ERR_INVALID_ARG,
             "dy_depth_to_space2_nhwc: views must be 16-byte aligned with pitches >= 4c / c");
  const int cp = c / epc;
  hipLaunchKernelGGL(depth_to_space2_kernel, dim3(mask_grid_for((long long)n * 4 * h * w * cp)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const u32x4*)src, (u32x4*)dst, n, 2 * h, 2 * w, cp, ld_src / epc, ld_dst / epc);
  return check_launch("depth_to_space2_kernel");
}

extern "C" int32_t dy_mask_gather(const dy_mask_gather_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->rows && d->counts && d->index && d->out, DY_ERR_INVALID_ARG, "dy_mask_gather: null pointer");
  DY_REQUIRE(d->nm == 32, DY_ERR_UNSUPPORTED, "dy_mask_gather: built for nm = 32 mask coefficients");
  DY_REQUIRE(d->batch > 0 && d->max_det > 0 && d->anchors > 0, DY_ERR_INVALID_ARG, "dy_mask_gather: bad dims");
  GatherArgs a;
  a.rows = d->rows, a.counts = d->counts, a.index = d->index, a.out = d->out;
  a.pred = d->pred, a.pred_ch = d->pred_ch, a.pred_c0 = d->pred_c0, a.anchors = d->anchors;
  a.batch = d->batch, a.max_det = d->max_det, a.nm = d->nm, a.n_levels = 0;
  for (int i = 0; i < DY_MAX_LEVELS; ++i) a.level[i] = nullptr, a.hw[i] = 0, a.ld[i] = 0, a.a0[i] = 0;
  a.a0[DY_MAX_LEVELS] = 0;
  if (d->pred) {
    DY_REQUIRE(d->pred_c0 >= 0 && d->pred_c0 + d->nm <= d->pred_ch, DY_ERR_INVALID_ARG, "dy_mask_gather: coefficient channels outside pred");
  } else {
    DY_REQUIRE(d->n_levels > 0 && d->n_levels <= DY_MAX_LEVELS, DY_ERR_INVALID_ARG, "dy_mask_gather: bad n_levels");
    long long A = 0;
    for (int i = 0; i < d->n_levels; ++i) {
      DY_REQUIRE(d->level[i] && d->h[i] > 0 && d->w[i] > 0 && d->ld[i] >= d->nm, DY_ERR_INVALID_ARG, "dy_mask_gather: bad level %d", i);
      a.level[i] = d->level[i], a.hw[i] = d->h[i] * d->w[i], a.ld[i] = d->ld[i], a.a0[i] = (int)A;
      A += (long long)d->h[i] * d->w[i];
    }
    DY_REQUIRE(A == d->anchors, DY_ERR_INVALID_ARG, "dy_mask_gather: the levels hold %lld anchors, anchors = %d", A, d->anchors);
    a.n_levels = d->n_levels;
    for (int i = d->n_levels; i <= DY_MAX_LEVELS; ++i) a.a0[i] = (int)A;
  }
  hipLaunchKernelGGL(mask_gather_kernel, dim3(mask_grid_for((long long)d->batch * d->max_det * (4 + d->nm))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return check_launch("mask_gather_kernel");
}

extern "C" int32_t dy_process_mask(const dy_process_mask_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->protos && d->side && d->counts && d->offsets && d->window, DY_ERR_INVALID_ARG, "dy_process_mask: null pointer");
  DY_REQUIRE(d->nm == 32, DY_ERR_UNSUPPORTED, "dy_process_mask: built for nm = 32 mask coefficients");
  DY_REQUIRE(d->batch > 0 && d->max_det > 0 && d->mh > 0 && d->mw > 0 && d->oh > 0 && d->ow > 0 && d->total >= 0, DY_ERR_INVALID_ARG, "dy_process_mask: bad dims");
  DY_REQUIRE(d->ld_p >= 32 && d->ld_p % 4 == 0 && aligned16(d->protos), DY_ERR_INVALID_ARG, "dy_process_mask: protos must be 16-byte aligned 128-byte rows");
  DY_REQUIRE(!d->crop_at_output || d->crop_rows, DY_ERR_INVALID_ARG, "dy_process_mask: crop_at_output needs crop_rows");
  DY_REQUIRE((long long)d->total <= (long long)d->batch * d->max_det, DY_ERR_INVALID_ARG, "dy_process_mask: total exceeds batch * max_det");
  if (d->total == 0) return DY_OK;
  DY_REQUIRE(d->out && (reinterpret_cast<uintptr_t>(d->out) & 7u) == 0, DY_ERR_INVALID_ARG, "dy_process_mask: out must be 8-byte aligned");
  const long long P = (long long)d->oh * d->ow;
  const long long gy = (P + kPixPerBlock - 1) / kPixPerBlock;
  DY_REQUIRE(gy <= 65535, DY_ERR_UNSUPPORTED, "dy_process_mask: output of %d x %d pixels is beyond the launch grid", d->oh, d->ow);
  PmArgs a;
  a.protos = d->protos, a.side = d->side, a.counts = d->counts, a.offsets = d->offsets, a.window = d->window, a.crop_rows = d->crop_rows;
  a.batch = d->batch, a.max_det = d->max_det, a.mh = d->mh, a.mw = d->mw, a.ld_p = d->ld_p, a.oh = d->oh, a.ow = d->ow, a.total = d->total;
  a.crop_at_output = d->crop_at_output ? 1 : 0, a.ratio_x = d->ratio_x, a.ratio_y = d->ratio_y, a.out = d->out;
  a.div_ow = make_fastdiv((unsigned)d->ow);
  hipLaunchKernelGGL(process_mask_kernel, dim3((unsigned)d->total, (unsigned)gy), dim3(kPmThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
  return check_launch("process_mask_kernel");
}

extern "C" int32_t dy_tile_process_mask(const dy_tile_process_mask_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->protos && d->side && d->counts && d->offsets_yx && d->owner && d->dest, DY_ERR_INVALID_ARG,
             "dy_tile_process_mask: null pointer (protos / side / counts / offsets_yx / owner / dest)");
  DY_REQUIRE(d->nm == 32, DY_ERR_UNSUPPORTED, "dy_tile_process_mask: built for nm = 32 mask coefficients");
  DY_REQUIRE(d->stride == 1 || d->stride == 2 || d->stride == 4, DY_ERR_UNSUPPORTED, "dy_tile_process_mask: stride %d (1, 2 or 4)", d->stride);
  DY_REQUIRE(d->frames > 0 && d->tiles > 0 && d->max_det > 0 && d->merge_max_det > 0 && d->mh > 0 && d->mw > 0 && d->tile_h > 0 && d->tile_w > 0 &&
                 d->frame_h > 0 && d->frame_w > 0 && d->total >= 0,
             DY_ERR_INVALID_ARG, "dy_tile_process_mask: bad dims");
  DY_REQUIRE((long long)d->mh * 4 == d->tile_h && (long long)d->mw * 4 == d->tile_w, DY_ERR_UNSUPPORTED,
             "dy_tile_process_mask: a proto grid of %d x %d is not a quarter of the %d x %d tile", d->mh, d->mw, d->tile_h, d->tile_w);
  DY_REQUIRE((long long)d->tiles * d->max_det <= TM_MAX_SLOTS, DY_ERR_UNSUPPORTED, "dy_tile_process_mask: tiles * max_det = %lld > %d",
             (long long)d->tiles * d->max_det, TM_MAX_SLOTS);
  DY_REQUIRE(d->merge_max_det <= TM_MAX_KEEP, DY_ERR_UNSUPPORTED, "dy_tile_process_mask: merge_max_det %d > %d", d->merge_max_det, TM_MAX_KEEP);
  DY_REQUIRE(d->frames <= 65535, DY_ERR_UNSUPPORTED, "dy_tile_process_mask: %d frames are beyond the launch grid", d->frames);
  DY_REQUIRE(d->tile_h < (1 << 20) && d->tile_w < (1 << 20) && d->frame_h < (1 << 20) && d->frame_w < (1 << 20), DY_ERR_INVALID_ARG,
             "dy_tile_process_mask: sides of 2^20 pixels and more are beyond the exact fp32 coordinates");
  DY_REQUIRE(d->ld_p >= 32 && d->ld_p % 4 == 0 && aligned16(d->protos), DY_ERR_INVALID_ARG,
             "dy_tile_process_mask: protos must be 16-byte aligned 128-byte rows");
  const int oh = (d->frame_h + d->stride - 1) / d->stride, ow = (d->frame_w + d->stride - 1) / d->stride;
  DY_REQUIRE((long long)oh * ow < (1ll << 31), DY_ERR_INVALID_ARG, "dy_tile_process_mask: masks of %d x %d pixels", oh, ow);
  DY_REQUIRE((long long)d->total <= (long long)d->frames * d->merge_max_det, DY_ERR_INVALID_ARG, "dy_tile_process_mask: total exceeds frames * merge_max_det");
  if (d->total == 0) return DY_OK;
  DY_REQUIRE(d->out && (reinterpret_cast<uintptr_t>(d->out) & 3u) == 0, DY_ERR_INVALID_ARG, "dy_tile_process_mask: out must be 4-byte aligned");
  TpmArgs a;
  a.protos = d->protos, a.side = d->side, a.counts = d->counts, a.offs = d->offsets_yx, a.owner = d->owner, a.dest = d->dest, a.out = d->out;
  a.K = d->tiles, a.max_det = d->max_det, a.N = d->tiles * d->max_det, a.keep = d->merge_max_det, a.mh = d->mh, a.mw = d->mw, a.ld_p = d->ld_p;
  a.th = d->tile_h, a.tw = d->tile_w, a.oh = oh, a.ow = ow, a.s = d->stride, a.total = d->total;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long long bytes = (long long)d->total * oh * ow;
  hipLaunchKernelGGL(tile_mask_zero_kernel, dim3(mask_grid_for(bytes / 16 + 1)), dim3(256), 0, st, d->out, bytes, aligned16(d->out) ? 1 : 0);
  // workgroups per live slot: a tile-sized region in steps of eight words a thread, at most 16
  const long long words = ((long long)d->tile_h / d->stride + 3) * (((long long)d->tile_w / d->stride + 3) / 4 + 2);
  long long gy = (words + kTpmThreads * 8 - 1) / (kTpmThreads * 8);
  gy = gy < 1 ? 1 : (gy > 16 ? 16 : gy);
  hipLaunchKernelGGL(tile_process_mask_kernel, dim3((unsigned)a.N, (unsigned)gy, (unsigned)d->frames), dim3(kTpmThreads), 0, st, a);
  return check_launch("tile_process_mask_kernel");
}
