// Segmentation training on the device (include/dyolo.h): dy_seg_loss, the mask term of the reference's v8SegmentationLoss (utils/loss.py:263-443:
// calculate_segmentation_loss, single_mask_loss; crop_mask, utils/ops.py:660-676; overlap_mask=True) with its gradient w.r.t. the mask
// coefficients and the prototypes, behind dy_detection_loss's owner map; and two small kernels of the Segment head's backward:
// dy_space_to_depth2_nhwc (the inverse of dy_depth_to_space2_nhwc) and dy_grad_cast_scaled (fp32 gradient rows -> the storage type, times
// a device scalar).
//
// Launch sequence: seg_compact (one workgroup per image: the image's positives in anchor order) -> seg_zero_rows (grad_coef written whole)
// -> seg_pos (pass A, one wave per positive over its crop: the term, d coef, and the positive's record) -> seg_proto_grad (pass B, one workgroup
// per 16 x 16 prototype tile over the image's records: d proto, stored once) -> seg_final (the value, summed in a fixed order).  No atomics:
// two calls on the same inputs give the same bits.  No dense (batch, n, mh, mw) tensor, nothing synchronises the host.
#include "common_hip.h"

namespace dy {

constexpr int kSegNm = 32;   // mask coefficients / prototype channels (Segment's nm in every YAML)
constexpr int kSegRec = 40;  // words of a positive's record: c0, c1, r0, r1 (int), weight (float), mask value (int), 2 unused, coef[32]
constexpr int kSegChunk = 128;  // record headers staged in LDS per round of pass B

struct SegLossArgs {
  const int* owner;
  const float* gt;
  const float* coef[DY_MAX_LEVELS];
  int h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS], a0[DY_MAX_LEVELS + 1];
  int n_levels, batch, A, gmax, cap;
  const void* proto;
  int ld_proto, mh, mw;
  const void* masks;
  int mask_i32, gh, gw, shift;
  float img_h, img_w, box_gain;
  int2* list;
  int* count;
  float* rec;
  float* term;
  float* out;
  float* gcoef[DY_MAX_LEVELS];
  int gld[DY_MAX_LEVELS];
  float* gproto;
  int ld_gproto;
};

// ---- ordered compaction: (anchor, label row) of every anchor with owner >= 0, in anchor order -------------------------------------------
__global__ __launch_bounds__(256) void seg_compact_kernel(const SegLossArgs p) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* ow = p.owner + (size_t)b * p.A;
  int2* list = p.list + (size_t)b * p.cap;
  int running = 0;
  for (int start = 0; start < p.A; start += 256) {
    const int a = start + tid;
    const int g = a < p.A ? ow[a] : -1;
    const bool fg = g >= 0 && g < p.gmax;
    const unsigned long long m = __ballot(fg);
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int off = running, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < wv) off += wsum[i];
      tot += wsum[i];
    }
    if (fg) {
      const int i = off + __popcll(m & ((1ull << lane) - 1ull));
      if (i < p.cap) list[i] = int2{a, g};
    }
    running += tot;
    __syncthreads();
  }
  if (tid == 0) p.count[b] = running < p.cap ? running : p.cap;
}

// grad_coef rows written whole: zeros everywhere, pass A then writes the positives' rows
__global__ __launch_bounds__(256) void seg_zero_rows_kernel(float* __restrict__ g, int ld, long long rows) {
  const long long total = rows * (kSegNm / 4);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
    *reinterpret_cast<float4*>(g + (i >> 3) * ld + (i & 7) * 4) = float4{0.f, 0.f, 0.f, 0.f};
}

template <typename T>
static __device__ __forceinline__ void seg_load_pixel(const T* __restrict__ q, float (&v)[kSegNm]) {
  constexpr int EPC = 16 / (int)sizeof(T);
#pragma unroll
  for (int c = 0; c < kSegNm / EPC; ++c) {
    const u32x4 raw = *reinterpret_cast<const u32x4*>(q + c * EPC);
    const T* t = reinterpret_cast<const T*>(&raw);
#pragma unroll
    for (int e = 0; e < EPC; ++e) v[c * EPC + e] = Elem<T>::to_f32(t[e]);
  }
}

static __device__ __forceinline__ int seg_mask_at(const SegLossArgs& p, int b, int py, int px) {
  const size_t i = ((size_t)b * p.gh + (py >> p.shift)) * p.gw + (px >> p.shift);
  return p.mask_i32 ? reinterpret_cast<const int*>(p.masks)[i] : (int)reinterpret_cast<const unsigned char*>(p.masks)[i];
}

// BCE with logits in its stable form and its derivative: l = max(z, 0) - z t + log(1 + exp(-|z|)), dl/dz = sigmoid(z) - t
static __device__ __forceinline__ void seg_bce(float z, float t, float* l, float* dz) {
  const float e = expf(-fabsf(z));
  *l = fmaxf(z, 0.f) - z * t + log1pf(e);
  const float r = 1.f / (1.f + e);
  *dz = (z >= 0.f ? r : e * r) - t;
}

static __device__ __forceinline__ float seg_dot(const float (&c)[kSegNm], const float (&v)[kSegNm]) {
  float z = 0.f;
#pragma unroll
  for (int k = 0; k < kSegNm; ++k) z = fmaf(c[k], v[k], z);
  return z;
}

static __device__ __forceinline__ int seg_nfg(const SegLossArgs& p) {
  int n = 0;
  for (int b = 0; b < p.batch; ++b) n += p.count[b];
  return n;
}

// first integer r with r >= v, clamped to [0, n]: for integer r, (r >= v) == (r >= ceil(v)) and (r < v) == (r < ceil(v))
static __device__ __forceinline__ int seg_edge(float v, int n) { return (int)fminf(fmaxf(ceilf(v), 0.f), (float)n); }

// ---- pass A: one wave per positive --------------------------------------------------------------------------------------------------------
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void seg_pos_kernel(const SegLossArgs p) {
  const int lane = threadIdx.x & 63;
  const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = (int)(gw / p.cap), i = (int)(gw - (long long)b * p.cap);
  if (b >= p.batch || i >= p.count[b]) return;
  const int2 ag = p.list[(size_t)b * p.cap + i];
  const int a = ag.x, g = ag.y;
  int l = 0;
  while (l + 1 < p.n_levels && a >= p.a0[l + 1]) ++l;
  const size_t row = (size_t)b * p.h[l] * p.w[l] + (a - p.a0[l]);
  const float* cr = p.coef[l] + row * (size_t)p.ld[l];
  float cf[kSegNm];
#pragma unroll
  for (int k = 0; k < kSegNm; k += 4) {
    const float4 v = *reinterpret_cast<const float4*>(cr + k);
    cf[k] = v.x, cf[k + 1] = v.y, cf[k + 2] = v.z, cf[k + 3] = v.w;
  }
  const float* box = p.gt + ((size_t)b * p.gmax + g) * 5;
  // loss.py:417-423: normalise by the image size, then scale to the prototype grid -- divide, then multiply, in fp32
  const float x1n = box[1] / p.img_w, y1n = box[2] / p.img_h, x2n = box[3] / p.img_w, y2n = box[4] / p.img_h;
  const float area = (x2n - x1n) * (y2n - y1n);
  const int c0 = seg_edge(x1n * (float)p.mw, p.mw), c1 = seg_edge(x2n * (float)p.mw, p.mw);
  const int r0 = seg_edge(y1n * (float)p.mh, p.mh), r1 = seg_edge(y2n * (float)p.mh, p.mh);
  const int cw = c1 > c0 ? c1 - c0 : 0, ch = r1 > r0 ? r1 - r0 : 0, npx = cw * ch;
  const T* pb = reinterpret_cast<const T*>(p.proto) + (size_t)b * p.mh * p.mw * p.ld_proto;
  float lsum = 0.f;
  float dc[kSegNm];
#pragma unroll
  for (int k = 0; k < kSegNm; ++k) dc[k] = 0.f;
  for (int idx = lane; idx < npx; idx += 64) {
    const int py = r0 + idx / cw, px = c0 + idx % cw;
    float v[kSegNm];
    seg_load_pixel<T>(pb + ((size_t)py * p.mw + px) * p.ld_proto, v);
    const float t = seg_mask_at(p, b, py, px) == g + 1 ? 1.f : 0.f;
    float lv, dz;
    seg_bce(seg_dot(cf, v), t, &lv, &dz);
    lsum += lv;
    if (GRAD) {
#pragma unroll
      for (int k = 0; k < kSegNm; ++k) dc[k] = fmaf(dz, v[k], dc[k]);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) lsum += __shfl_xor(lsum, off);
  const double norm = (double)p.mh * (double)p.mw * (double)area;
  if (lane == 0) p.term[(size_t)b * p.cap + i] = (float)((double)lsum / norm);
  if (GRAD) {
    const int nfg = seg_nfg(p);  // >= 1 here
    const float wgt = (float)((double)p.box_gain * (double)p.batch / (double)nfg / norm);  // d total / d (sum of the crop's BCE)
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < kSegNm; ++k) {
      float s = dc[k];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
      if (lane == k) mine = s;
    }
    float mycf = 0.f;
#pragma unroll
    for (int k = 0; k < kSegNm; ++k)
      if (lane == k) mycf = cf[k];
    float* rec = p.rec + ((size_t)b * p.cap + i) * kSegRec;
    if (lane < kSegNm) {
      p.gcoef[l][row * (size_t)p.gld[l] + lane] = mine * wgt;
      rec[8 + lane] = mycf;
    }
    if (lane == 0) {
      int* ri = reinterpret_cast<int*>(rec);
      ri[0] = c0, ri[1] = c0 + cw, ri[2] = r0, ri[3] = r0 + ch;
      rec[4] = wgt;
      ri[5] = g + 1, ri[6] = 0, ri[7] = 0;
    }
  }
}

// ---- pass B: one workgroup per 16 x 16 prototype tile ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void seg_proto_grad_kernel(const SegLossArgs p) {
  __shared__ int hdr[kSegChunk * 8];
  const int b = blockIdx.z, tx0 = blockIdx.x * 16, ty0 = blockIdx.y * 16;
  const int px = tx0 + (threadIdx.x & 15), py = ty0 + (threadIdx.x >> 4);
  const bool in = px < p.mw && py < p.mh;
  float v[kSegNm], acc[kSegNm];
#pragma unroll
  for (int k = 0; k < kSegNm; ++k) v[k] = 0.f, acc[k] = 0.f;
  int mv = 0;
  if (in) {
    seg_load_pixel<T>(reinterpret_cast<const T*>(p.proto) + (((size_t)b * p.mh + py) * p.mw + px) * p.ld_proto, v);
    mv = seg_mask_at(p, b, py, px);
  }
  const int cnt = p.count[b];
  const float* recs = p.rec + (size_t)b * p.cap * kSegRec;
  for (int start = 0; start < cnt; start += kSegChunk) {
    const int nrec = cnt - start < kSegChunk ? cnt - start : kSegChunk;
    __syncthreads();
    for (int t = threadIdx.x; t < nrec * 8; t += 256) hdr[t] = reinterpret_cast<const int*>(recs)[(size_t)(start + (t >> 3)) * kSegRec + (t & 7)];
    __syncthreads();
    for (int j = 0; j < nrec; ++j) {
      const int c0 = hdr[j * 8], c1 = hdr[j * 8 + 1], r0 = hdr[j * 8 + 2], r1 = hdr[j * 8 + 3];
      if (c1 <= tx0 || c0 >= tx0 + 16 || r1 <= ty0 || r0 >= ty0 + 16) continue;  // the same for every thread of the workgroup
      if (in && px >= c0 && px < c1 && py >= r0 && py < r1) {
        const float* cr = recs + (size_t)(start + j) * kSegRec + 8;
        float cf[kSegNm];
#pragma unroll
        for (int k = 0; k < kSegNm; k += 4) {
          const float4 q = *reinterpret_cast<const float4*>(cr + k);
          cf[k] = q.x, cf[k + 1] = q.y, cf[k + 2] = q.z, cf[k + 3] = q.w;
        }
        float lv, dz;
        seg_bce(seg_dot(cf, v), mv == hdr[j * 8 + 5] ? 1.f : 0.f, &lv, &dz);
        const float f = dz * __int_as_float(hdr[j * 8 + 4]);
#pragma unroll
        for (int k = 0; k < kSegNm; ++k) acc[k] = fmaf(f, cf[k], acc[k]);
      }
    }
  }
  if (in) {
    float* o = p.gproto + (((size_t)b * p.mh + py) * p.mw + px) * p.ld_gproto;
#pragma unroll
    for (int k = 0; k < kSegNm; k += 4) *reinterpret_cast<float4*>(o + k) = float4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
  }
}

// ---- the value: the positives' terms summed in a fixed order, in double ---------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_final_kernel(const SegLossArgs p) {
  __shared__ double part[256];
  double s = 0.0;
  int nfg = 0;
  for (int b = 0; b < p.batch; ++b) {
    const int cnt = p.count[b];
    nfg += cnt;
    for (int i = threadIdx.x; i < cnt; i += 256) s += (double)p.term[(size_t)b * p.cap + i];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double seg = nfg > 0 ? (double)p.box_gain * part[0] / (double)nfg : 0.0;
    p.out[0] = (float)seg;
    p.out[1] = (float)(seg * (double)p.batch);
  }
}

// ---- dy_space_to_depth2_nhwc: one 16-byte chunk per thread (grid-stride); cp = chunks per SOURCE pixel ------------------------------------
__global__ __launch_bounds__(256) void space_to_depth2_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int n, int hs, int ws, int cp, int lds_c,
                                                              int ldd_c) {
  const long long total = (long long)n * hs * ws * cp;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % cp);
    long long q = i / cp;
    const int sx = (int)(q % ws);
    q /= ws;
    const int sy = (int)(q % hs);
    const long long b = q / hs;
    const int sub = ((sy & 1) << 1) | (sx & 1);
    const long long dp = (b * (hs >> 1) + (sy >> 1)) * (ws >> 1) + (sx >> 1);
    dst[dp * ldd_c + sub * cp + k] = src[((b * hs + sy) * ws + sx) * lds_c + k];
  }
}

// ---- dy_grad_cast_scaled: eight channels per thread ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void grad_cast_scaled_kernel(const float* __restrict__ g, int ld_g, long long rows, int c8, const float* __restrict__ scale,
                                                               T* __restrict__ dz, int ld_dz) {
  const float s = scale ? *scale : 1.f;
  const long long total = rows * c8;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / c8;
    const int k = (int)(i - r * c8) * 8;
    const float4 lo = *reinterpret_cast<const float4*>(g + r * ld_g + k), hi = *reinterpret_cast<const float4*>(g + r * ld_g + k + 4);
    const float f[8] = {lo.x * s, lo.y * s, lo.z * s, lo.w * s, hi.x * s, hi.y * s, hi.z * s, hi.w * s};
    T* o = dz + r * ld_dz + k;
    if (sizeof(T) == 2) {
      T t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = Elem<T>::from_f32(f[e]);
      *reinterpret_cast<u32x4*>(o) = *reinterpret_cast<const u32x4*>(t);
    } else {
      *reinterpret_cast<float4*>(o) = float4{f[0], f[1], f[2], f[3]};
      *reinterpret_cast<float4*>(o + 4) = float4{f[4], f[5], f[6], f[7]};
    }
  }
}

static inline size_t salign(size_t v) { return (v + 255) / 256 * 256; }
static inline long long seg_cap(long long anchors, long long gmax, long long topk) { return anchors < gmax * topk ? anchors : gmax * topk; }
static inline unsigned seg_grid(long long total, long long limit = 8192) {
  long long g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > limit ? limit : g));
}

}  // namespace dy

using namespace dy;

extern "C" int64_t dy_seg_loss_workspace_bytes(int32_t batch, int32_t anchors, int32_t gmax, int32_t topk) {
  if (batch <= 0 || anchors <= 0 || gmax < 0 || topk <= 0) return -1;
  const size_t bc = (size_t)batch * (size_t)(seg_cap(anchors, gmax, topk) > 0 ? seg_cap(anchors, gmax, topk) : 1);
  return (int64_t)(salign(bc * 8) + salign((size_t)batch * 4) + salign(bc * kSegRec * 4) + salign(bc * 4));
}

extern "C" int32_t dy_seg_loss(const dy_seg_loss_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->out && d->workspace && d->owner && d->proto && d->masks, DY_ERR_INVALID_ARG, "dy_seg_loss: null pointer");
  DY_REQUIRE(d->n_levels >= 1 && d->n_levels <= DY_MAX_LEVELS && d->batch > 0 && d->gmax >= 0 && d->topk > 0 && d->mh > 0 && d->mw > 0 && d->gh > 0 && d->gw > 0,
             DY_ERR_INVALID_ARG, "dy_seg_loss: bad dims");
  DY_REQUIRE(d->nm == kSegNm, DY_ERR_UNSUPPORTED, "dy_seg_loss: nm %d not built (only %d)", d->nm, kSegNm);
  DY_REQUIRE(d->gmax == 0 || d->gt, DY_ERR_INVALID_ARG, "dy_seg_loss: gt is null");
  DY_REQUIRE(d->img_h > 0.f && d->img_w > 0.f, DY_ERR_INVALID_ARG, "dy_seg_loss: the image size is not positive");
  const int ratio = d->mh / d->gh;
  DY_REQUIRE((ratio == 1 || ratio == 2) && d->gh * ratio == d->mh && d->gw * ratio == d->mw, DY_ERR_UNSUPPORTED,
             "dy_seg_loss: a %d x %d index map under a %d x %d prototype grid (the grid must equal the map or be exactly twice it)", d->gh, d->gw, d->mh, d->mw);
  DY_REQUIRE(d->mask_dtype == DY_MASK_U8 || d->mask_dtype == DY_MASK_I32, DY_ERR_UNSUPPORTED, "dy_seg_loss: index maps are uint8 or int32");
  DY_REQUIRE(d->mask_dtype == DY_MASK_I32 || d->gmax <= 255, DY_ERR_UNSUPPORTED, "dy_seg_loss: %d label rows do not fit a uint8 index map", d->gmax);
  const int es = dtype_size_no_fp8(d->proto_dtype);
  DY_REQUIRE(es == 2 || es == 4, DY_ERR_UNSUPPORTED, "dy_seg_loss: prototypes are bf16, f16 or f32");
  DY_REQUIRE(d->ld_proto >= kSegNm && (d->ld_proto * es) % 16 == 0 && aligned16(d->proto), DY_ERR_INVALID_ARG,
             "dy_seg_loss: prototype rows must hold %d channels in whole 16-byte chunks", kSegNm);
  SegLossArgs a{};
  long long A = 0;
  const bool want_grad = d->grad_proto != nullptr;
  for (int i = 0; i < d->n_levels; ++i) {
    DY_REQUIRE(d->coef[i] && d->h[i] > 0 && d->w[i] > 0 && d->ld_coef[i] >= kSegNm && d->ld_coef[i] % 4 == 0 && aligned16(d->coef[i]), DY_ERR_INVALID_ARG,
               "dy_seg_loss: coefficient level %d invalid", i);
    a.coef[i] = d->coef[i];
    a.h[i] = d->h[i];
    a.w[i] = d->w[i];
    a.ld[i] = d->ld_coef[i];
    a.a0[i] = (int)A;
    A += (long long)d->h[i] * d->w[i];
    DY_REQUIRE(A * d->batch < (1ll << 29), DY_ERR_UNSUPPORTED, "dy_seg_loss: too many anchors for 32-bit indices");
    if (want_grad) {
      DY_REQUIRE(d->grad_coef[i] && d->ld_grad_coef[i] >= kSegNm && d->ld_grad_coef[i] % 4 == 0 && aligned16(d->grad_coef[i]), DY_ERR_INVALID_ARG,
                 "dy_seg_loss: grad_coef level %d invalid", i);
      a.gcoef[i] = d->grad_coef[i];
      a.gld[i] = d->ld_grad_coef[i];
    }
  }
  if (want_grad)
    DY_REQUIRE(d->ld_grad_proto >= kSegNm && d->ld_grad_proto % 4 == 0 && aligned16(d->grad_proto), DY_ERR_INVALID_ARG, "dy_seg_loss: grad_proto invalid");
  DY_REQUIRE((long long)d->batch * d->mh * d->mw < (1ll << 31), DY_ERR_UNSUPPORTED, "dy_seg_loss: prototype grid too large");
  a.a0[d->n_levels] = (int)A;
  a.n_levels = d->n_levels;
  a.batch = d->batch;
  a.A = (int)A;
  a.gmax = d->gmax;
  const long long cap = seg_cap(A, d->gmax, d->topk) > 0 ? seg_cap(A, d->gmax, d->topk) : 1;
  a.cap = (int)cap;
  a.owner = d->owner;
  a.gt = d->gt;
  a.proto = d->proto;
  a.ld_proto = d->ld_proto;
  a.mh = d->mh;
  a.mw = d->mw;
  a.masks = d->masks;
  a.mask_i32 = d->mask_dtype == DY_MASK_I32;
  a.gh = d->gh;
  a.gw = d->gw;
  a.shift = ratio - 1;
  a.img_h = d->img_h;
  a.img_w = d->img_w;
  a.box_gain = d->box_gain;
  a.out = d->out;
  a.gproto = d->grad_proto;
  a.ld_gproto = d->ld_grad_proto;
  const int64_t need = dy_seg_loss_workspace_bytes(d->batch, (int)A, d->gmax, d->topk);
  DY_REQUIRE(d->workspace_bytes >= need && aligned16(d->workspace), DY_ERR_WORKSPACE, "dy_seg_loss: workspace %lld < %lld bytes", (long long)d->workspace_bytes,
             (long long)need);
  unsigned char* ws = reinterpret_cast<unsigned char*>(d->workspace);
  const size_t bc = (size_t)d->batch * (size_t)cap;
  a.list = reinterpret_cast<int2*>(ws);
  ws += salign(bc * 8);
  a.count = reinterpret_cast<int*>(ws);
  ws += salign((size_t)d->batch * 4);
  a.rec = reinterpret_cast<float*>(ws);
  ws += salign(bc * kSegRec * 4);
  a.term = reinterpret_cast<float*>(ws);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(seg_compact_kernel, dim3((unsigned)d->batch), dim3(256), 0, st, a);
  if (want_grad)
    for (int i = 0; i < d->n_levels; ++i) {
      const long long rows = (long long)d->batch * d->h[i] * d->w[i];
      hipLaunchKernelGGL(seg_zero_rows_kernel, dim3(seg_grid(rows * (kSegNm / 4))), dim3(256), 0, st, a.gcoef[i], a.gld[i], rows);
    }
  const long long waves = (long long)d->batch * cap;
  DY_REQUIRE((waves + 3) / 4 < (1ll << 31), DY_ERR_UNSUPPORTED, "dy_seg_loss: too many label rows");
  const dim3 ga((unsigned)((waves + 3) / 4)), gb((unsigned)((d->mw + 15) / 16), (unsigned)((d->mh + 15) / 16), (unsigned)d->batch);
  DY_REQUIRE(d->batch <= 65535 && gb.y <= 65535, DY_ERR_UNSUPPORTED, "dy_seg_loss: batch / grid too large for one launch");
#define SEG_LAUNCH(T)                                                                                      \
  do {                                                                                                     \
    if (want_grad) {                                                                                       \
      hipLaunchKernelGGL((seg_pos_kernel<T, true>), ga, dim3(256), 0, st, a);                              \
      hipLaunchKernelGGL((seg_proto_grad_kernel<T>), gb, dim3(256), 0, st, a);                             \
    } else {                                                                                               \
      hipLaunchKernelGGL((seg_pos_kernel<T, false>), ga, dim3(256), 0, st, a);                             \
    }                                                                                                      \
  } while (0)
  if (d->proto_dtype == DY_BF16) SEG_LAUNCH(bf16_t);
  else if (d->proto_dtype == DY_F16) SEG_LAUNCH(f16_t);
  else SEG_LAUNCH(float);
#undef SEG_LAUNCH
  hipLaunchKernelGGL(seg_final_kernel, dim3(1), dim3(256), 0, st, a);
  return check_launch("dy_seg_loss");
}

extern "C" int32_t dy_space_to_depth2_nhwc(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_src, int32_t ld_dst, int32_t dtype,
                                           dy_stream_t stream) {
  const int es = dy_dtype_size(dtype);
  DY_REQUIRE(src && dst && es && dtype != DY_FP8, DY_ERR_INVALID_ARG, "dy_space_to_depth2_nhwc: null pointer or bad dtype");
  DY_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, DY_ERR_INVALID_ARG, "dy_space_to_depth2_nhwc: bad dims");
  DY_REQUIRE(c % 8 == 0, DY_ERR_UNSUPPORTED, "dy_space_to_depth2_nhwc: c must be a multiple of 8 (whole 16-byte chunks in every storage type)");
  const int epc = 16 / es;
  DY_REQUIRE(aligned16(src) && aligned16(dst) && ld_src % epc == 0 && ld_dst % epc == 0 && ld_src >= c && ld_dst >= 4 * c, DY_ERR_INVALID_ARG,
             "dy_space_to_depth2_nhwc: views must be 16-byte aligned with pitches >= c / 4c");
  const int cp = c / epc;
  hipLaunchKernelGGL(space_to_depth2_kernel, dim3(seg_grid((long long)n * 4 * h * w * cp, 65536)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const u32x4*>(src), reinterpret_cast<u32x4*>(dst), n, 2 * h, 2 * w, cp, ld_src / epc, ld_dst / epc);
  return check_launch("space_to_depth2_kernel");
}

extern "C" int32_t dy_grad_cast_scaled(const float* g, int32_t ld_g, int64_t rows, int32_t c, const float* scale, void* dz, int32_t ld_dz, int32_t dtype,
                                       dy_stream_t stream) {
  const int es = dtype_size_no_fp8(dtype);
  DY_REQUIRE(g && dz && rows > 0 && c > 0 && (es == 2 || es == 4), DY_ERR_INVALID_ARG, "dy_grad_cast_scaled: bad arguments");
  DY_REQUIRE(c % 8 == 0, DY_ERR_UNSUPPORTED, "dy_grad_cast_scaled: c must be a multiple of 8");
  DY_REQUIRE(ld_g >= c && ld_g % 4 == 0 && aligned16(g) && ld_dz >= c && (ld_dz * es) % 16 == 0 && aligned16(dz), DY_ERR_INVALID_ARG,
             "dy_grad_cast_scaled: rows must hold c channels in whole 16-byte chunks");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned grid = seg_grid((long long)rows * (c / 8));
  if (dtype == DY_BF16) hipLaunchKernelGGL((grad_cast_scaled_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, g, ld_g, (long long)rows, c / 8, scale, (bf16_t*)dz, ld_dz);
  else if (dtype == DY_F16) hipLaunchKernelGGL((grad_cast_scaled_kernel<f16_t>), dim3(grid), dim3(256), 0, st, g, ld_g, (long long)rows, c / 8, scale, (f16_t*)dz, ld_dz);
  else hipLaunchKernelGGL((grad_cast_scaled_kernel<float>), dim3(grid), dim3(256), 0, st, g, ld_g, (long long)rows, c / 8, scale, (float*)dz, ld_dz);
  return check_launch("dy_grad_cast_scaled");
}
