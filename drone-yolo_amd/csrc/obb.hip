// Oriented boxes behind the Detect kernels: the prediction half of the reference's `obb` task.
//
//   dy_obb_decode     OBB.forward's angle (nn/modules/head.py:217-221: (sigmoid(logit) - 0.25) * pi) and dist2rbox (utils/tal.py).  Detect's
//                     own decode already wrote cx = (ax + xf) s, cy = (ay + yf) s and wh; the rotated centre is that centre turned about the
//                     anchor point a s:  (x, y) = a s + R(theta) ((cx, cy) - a s).  One thread per anchor, accesses coalesced along A.
//   dy_nms_rotated    non_max_suppression(rotated=True) for the single-label path (utils/ops.py:257-313) with nms_rotated (:146-178) and
//                     batch_probiou (utils/metrics.py:178-275).  The candidate stage (filter, keys, sort order, max_nms) is dy_nms's
//                     (nms_core.h); the suppression is the reference's FAST NMS, not the greedy scan of nms.hip.
//   dy_nms_rotated_ml the validator's form (multi_label: every (anchor, class) pair above conf is a candidate), an entry point of its own beside it.
//   dy_scale_rboxes   OBBPredictor.construct_result (models/yolo/obb/predict.py:43-45): regularize_rboxes + scale_boxes(xywh=True).
//
// fp32 in the reference's order of operations with contraction off.  expf / logf / sinf / cosf are the device's and are not bit-equal to
// the CPU's: kept sets agree for inputs the reference decides with a margin (tools/make_obb_golden.py records it).
#include "nms_core.h"
#include "probiou.h"

#pragma clang fp contract(off)

namespace dy {

constexpr float kPi = 3.14159265358979323846f;  // math.pi rounded to fp32, as torch rounds a Python scalar beside an fp32 tensor

// ---- dy_obb_decode ----------------------------------------------------------------------------------------------------------------
struct ObbDecodeArgs {
  const float* level[DY_MAX_LEVELS];
  int h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS], a0[DY_MAX_LEVELS + 1];  // a0: first anchor of the level
  float stride[DY_MAX_LEVELS];
  int n_levels, batch, nch, A;
  float* pred;
  float* theta;
};

// Memory-bound: per anchor one strided logit read, cx and cy read and written, theta written (24 B).  Lane = anchor, so the pred and
// theta accesses of a wave are 256 contiguous bytes each; the grid is capped and strides over the rest.
__global__ __launch_bounds__(256) void obb_decode_kernel(const ObbDecodeArgs p) {
  const long long total = (long long)p.batch * p.A;
  const long long step = (long long)gridDim.x * 256;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += step) {
    const int b = (int)(idx / p.A);
    const int a = (int)(idx - (long long)b * p.A);
    int l = 0;
    while (l + 1 < p.n_levels && a >= p.a0[l + 1]) ++l;
    const int pix = a - p.a0[l];
    const int row = pix / p.w[l], col = pix - row * p.w[l];
    const float logit = p.level[l][((size_t)b * p.h[l] * p.w[l] + pix) * (size_t)p.ld[l]];
    const float th = (1.f / (1.f + expf(-logit)) - 0.25f) * kPi;
    const float s = p.stride[l];
    const float ax = ((float)col + 0.5f) * s, ay = ((float)row + 0.5f) * s;
    float* px = p.pred + (size_t)b * p.nch * (size_t)p.A + a;
    float* py = px + p.A;
    const float dx = *px - ax, dy = *py - ay;
    const float cs = cosf(th), sn = sinf(th);
    *px = (dx * cs - dy * sn) + ax;
    *py = (dx * sn + dy * cs) + ay;
    p.theta[idx] = th;
  }
}

// ---- dy_nms_rotated ---------------------------------------------------------------------------------------------------------------
constexpr int RNMS_THREADS = 1024;
constexpr int RNMS_WAVES = RNMS_THREADS / 64;
constexpr int RNMS_LDS_CAP = 2048;  // candidates whose keys and table rows fit the kernel's LDS (56 KB); more: the workspace

struct RNmsArgs {
  NmsArgs n;
  const float* theta;  // [batch][A]
  float* table;        // [batch][5][cap]: the table of the images with more than RNMS_LDS_CAP candidates (cap = A, or A * nc with multi)
};

// One workgroup per image.  Sort as in nms.hip; then the five floats of every candidate (x + c, y + c and the covariance terms a, b, c)
// are computed once into a table, in LDS for at most RNMS_LDS_CAP candidates and in the workspace for more (decided here, on the device,
// like NMS_SMALL_CAP).  Candidates are resolved 64 at a time: wave w of a round takes chunk w of the round's 16, and each lane tests its
// candidate j against ALL table rows i < j, suppressed or not (ops.py:164-167: triu_(1), (ious >= thr).sum(0) <= 0).  A candidate's
// verdict depends on the table alone, so there is no serial dependence between chunks; only the position of a kept row (a prefix count
// of the kept bits) and the stop at max_det kept (ops.py:313) tie the rounds together.
// MULTI (dy_nms_rotated_ml, the validator's multi_label form): a candidate is an (anchor, class) pair whose key low word is anchor * nc +
// class; anchor and class both come from the key (the multi-label filter does not write p.cls), and the workspace table's pitch is the
// candidate capacity A * nc.
template <bool LDS, bool MULTI = false>
__device__ __forceinline__ void rnms_image(const RNmsArgs& q, int b, int n, u64* skeys, float* stab, u64* kmask) {
  const NmsArgs& p = q.n;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  u64* gkeys = p.keys + (size_t)b * p.P;
  const int tcap = MULTI ? p.cap : p.A;
  float* gtab = q.table + (size_t)b * 5 * (size_t)tcap;
  int P2 = 1;
  while (P2 < n) P2 <<= 1;
  if (LDS) {
    for (int i = tid; i < P2; i += RNMS_THREADS) skeys[i] = i < n ? gkeys[i] : ~0ull;
    __syncthreads();
    nms_bitonic_sort<RNMS_THREADS>(skeys, P2, tid);
  } else {
    for (int i = n + tid; i < P2; i += RNMS_THREADS) gkeys[i] = ~0ull;
    __syncthreads();
    nms_bitonic_sort<RNMS_THREADS>(gkeys, P2, tid);
  }
  const int nn = n < p.max_nms ? n : p.max_nms;
  const int ts = LDS ? RNMS_LDS_CAP : tcap;  // pitch of the table's five arrays
  const float* pr = p.pred + (size_t)b * p.nch * (size_t)p.A;
  const float* th = q.theta + (size_t)b * p.A;
  for (int i = tid; i < nn; i += RNMS_THREADS) {
    const int low = (int)(unsigned)((LDS ? skeys[i] : gkeys[i]) & 0xffffffffull);
    const int anchor = MULTI ? low / p.nc : low;
    const float off = p.agnostic ? 0.f : (MULTI ? (float)(low % p.nc) : (float)p.cls[(size_t)b * p.A + anchor]) * p.max_wh;
    const RRow r = rnms_row(pr[anchor] + off, pr[(size_t)p.A + anchor] + off, pr[(size_t)2 * p.A + anchor], pr[(size_t)3 * p.A + anchor], th[anchor]);
    float* t = LDS ? stab : gtab;
    t[i] = r.x;
    t[ts + i] = r.y;
    t[2 * ts + i] = r.a;
    t[3 * ts + i] = r.b;
    t[4 * ts + i] = r.c;
  }
  __syncthreads();

  float* outb = p.out + (size_t)b * p.max_det * 7;
  int nk = 0;
  for (int s0 = 0; s0 < nn && nk < p.max_det; s0 += RNMS_THREADS) {
    const int j = s0 + tid;
    const bool in = j < nn;
    const float* t = LDS ? stab : gtab;
    RRow me{0.f, 0.f, 0.f, 0.f, 0.f};
    if (in) me = RRow{t[j], t[ts + j], t[2 * ts + j], t[3 * ts + j], t[4 * ts + j]};
    bool sup = false;
    int iend = s0 + wave * 64 + 63;  // rows in front of the chunk's last candidate (wave-uniform)
    if (iend > nn) iend = nn;
    for (int i = 0; i < iend; ++i) {
      const RRow r{t[i], t[ts + i], t[2 * ts + i], t[3 * ts + i], t[4 * ts + i]};  // one address per wave: a broadcast read
      if (i < j && rnms_probiou(r, me) >= p.iou) sup = true;
      if ((i & 63) == 63 && __ballot(in && !sup) == 0ull) break;  // nothing of the chunk is left to decide
    }
    const u64 km = __ballot(in && !sup);
    if (lane == 0) kmask[wave] = km;
    __syncthreads();
    int base = nk, tot = 0;
    for (int w = 0; w < RNMS_WAVES; ++w) {
      const int c = __popcll(kmask[w]);
      if (w < wave) base += c;
      tot += c;
    }
    if (in && !sup) {
      const int at = base + __popcll(km & ((1ull << lane) - 1ull));
      if (at < p.max_det) {
        const u64 key = LDS ? skeys[j] : gkeys[j];
        const int low = (int)(unsigned)(key & 0xffffffffull);
        const int anchor = MULTI ? low / p.nc : low;
        float* o = outb + (size_t)at * 7;
        o[0] = pr[anchor];
        o[1] = pr[(size_t)p.A + anchor];
        o[2] = pr[(size_t)2 * p.A + anchor];
        o[3] = pr[(size_t)3 * p.A + anchor];
        o[4] = th[anchor];
        o[5] = __uint_as_float(~(unsigned)(key >> 32));
        o[6] = MULTI ? (float)(low % p.nc) : (float)p.cls[(size_t)b * p.A + anchor];
        if (p.out_index) p.out_index[(size_t)b * p.max_det + at] = anchor;
      }
    }
    nk += tot;
    __syncthreads();  // kmask may be rewritten
  }
  if (nk > p.max_det) nk = p.max_det;
  for (int r = nk * 7 + tid; r < p.max_det * 7; r += RNMS_THREADS) outb[r] = 0.f;
  if (p.out_index)
    for (int r = nk + tid; r < p.max_det; r += RNMS_THREADS) p.out_index[(size_t)b * p.max_det + r] = -1;
  if (tid == 0) p.out_count[b] = nk;
}

__global__ __launch_bounds__(RNMS_THREADS) void nms_rotated_kernel(const RNmsArgs q) {
  __shared__ u64 skeys[RNMS_LDS_CAP];
  __shared__ float stab[5 * RNMS_LDS_CAP];
  __shared__ u64 kmask[RNMS_WAVES];
  const int b = blockIdx.x;
  int n = q.n.counts[b];
  if (n > q.n.cap) n = q.n.cap;
  if (n <= RNMS_LDS_CAP) rnms_image<true>(q, b, n, skeys, stab, kmask);
  else rnms_image<false>(q, b, n, skeys, stab, kmask);
}

__global__ __launch_bounds__(RNMS_THREADS) void nms_rotated_ml_kernel(const RNmsArgs q) {
  __shared__ u64 skeys[RNMS_LDS_CAP];
  __shared__ float stab[5 * RNMS_LDS_CAP];
  __shared__ u64 kmask[RNMS_WAVES];
  const int b = blockIdx.x;
  int n = q.n.counts[b];
  if (n > q.n.cap) n = q.n.cap;
  if (n <= RNMS_LDS_CAP) rnms_image<true, true>(q, b, n, skeys, stab, kmask);
  else rnms_image<false, true>(q, b, n, skeys, stab, kmask);
}

// ---- dy_scale_rboxes --------------------------------------------------------------------------------------------------------------
// Python's / torch's `%` for a positive divisor: the remainder takes the divisor's sign
__device__ __forceinline__ float py_mod(float a, float m) {
  float r = fmodf(a, m);
  if (r != 0.f && r < 0.f) r += m;
  return r;
}

// regularize_rboxes (utils/ops.py:791-807), then scale_boxes(..., xywh=True) (:92-127): the pad is taken from x and y only, all four are
// divided by the gain, and clip_boxes (:335-354) clamps columns 0 and 2 to [0, w0] and columns 1 and 3 to [0, h0] -- for xywh rows that
// clamps the WIDTH and HEIGHT to the image as well.  This is the reference's behaviour and is reproduced as it is.
__global__ __launch_bounds__(256) void scale_rboxes_kernel(float* __restrict__ rows, const int* __restrict__ counts,
                                                           const float* __restrict__ params, int batch, int max_det) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= batch * max_det) return;
  const int b = idx / max_det, r = idx - b * max_det;
  if (r >= counts[b]) return;
  const float gain = params[b * 5], px = params[b * 5 + 1], py = params[b * 5 + 2];
  const float cw = params[b * 5 + 3], ch = params[b * 5 + 4];
  float* o = rows + (size_t)idx * 7;
  const float t = o[4];
  const bool swap = py_mod(t, kPi) >= kPi / 2.f;
  const float w = swap ? o[3] : o[2], h = swap ? o[2] : o[3];
  o[0] = fminf(fmaxf((o[0] - px) / gain, 0.f), cw);
  o[1] = fminf(fmaxf((o[1] - py) / gain, 0.f), ch);
  o[2] = fminf(fmaxf(w / gain, 0.f), cw);
  o[3] = fminf(fmaxf(h / gain, 0.f), ch);
  o[4] = py_mod(t, kPi / 2.f);
}

static inline size_t rnms_table_offset(int batch, int anchors) { return nms_align_up(nms_ws_bytes(batch, anchors), 256); }

}  // namespace dy

using namespace dy;

extern "C" int32_t dy_obb_decode(const dy_obb_decode_desc* d, dy_stream_t stream) {
  DY_REQUIRE(d && d->pred && d->theta, DY_ERR_INVALID_ARG, "dy_obb_decode: null pointer");
  DY_REQUIRE(d->n_levels >= 1 && d->n_levels <= DY_MAX_LEVELS && d->batch > 0 && d->nc > 0 && d->n_extra >= 0, DY_ERR_INVALID_ARG,
             "dy_obb_decode: bad dims");
  ObbDecodeArgs a{};
  long long A = 0;
  for (int i = 0; i < d->n_levels; ++i) {
    DY_REQUIRE(d->level[i] != nullptr, DY_ERR_INVALID_ARG, "dy_obb_decode: level %d is null", i);
    DY_REQUIRE(d->h[i] > 0 && d->w[i] > 0 && d->ld[i] >= 1 && d->stride[i] > 0.f, DY_ERR_INVALID_ARG, "dy_obb_decode: bad level %d", i);
    a.level[i] = d->level[i];
    a.h[i] = d->h[i];
    a.w[i] = d->w[i];
    a.ld[i] = d->ld[i];
    a.stride[i] = d->stride[i];
    a.a0[i] = (int)A;
    A += (long long)d->h[i] * d->w[i];
    DY_REQUIRE(A < (1ll << 30), DY_ERR_UNSUPPORTED, "dy_obb_decode: more than 2^30 anchors");
  }
  a.a0[d->n_levels] = (int)A;
  DY_REQUIRE(A == d->anchors, DY_ERR_INVALID_ARG, "dy_obb_decode: the levels hold %lld anchors, pred has %d", A, d->anchors);
  a.n_levels = d->n_levels;
  a.batch = d->batch;
  a.nch = 4 + d->nc + d->n_extra;
  a.A = d->anchors;
  a.pred = d->pred;
  a.theta = d->theta;
  long long blocks = ((long long)d->batch * d->anchors + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(obb_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return check_launch("obb_decode_kernel");
}

extern "C" int64_t dy_nms_rotated_workspace_bytes(int32_t batch, int32_t anchors) {
  if (batch <= 0 || anchors <= 0) return -1;
  return (int64_t)(rnms_table_offset(batch, anchors) + (size_t)batch * 5 * (size_t)anchors * 4);
}

extern "C" int32_t dy_nms_rotated(const dy_nms_desc* d, const float* theta, dy_stream_t stream) {
  DY_REQUIRE(d && theta, DY_ERR_INVALID_ARG, "dy_nms_rotated: null pointer");
  DY_REQUIRE(d->multi_label == 0, DY_ERR_UNSUPPORTED, "dy_nms_rotated: multi_label (the validator's NMS) is not built for rotated boxes");
  RNmsArgs q{};
  const int64_t extra = d->batch > 0 && d->anchors > 0
                            ? dy_nms_rotated_workspace_bytes(d->batch, d->anchors) - (int64_t)nms_ws_bytes(d->batch, d->anchors)
                            : 0;
  const int rc0 = nms_args_from_desc(d, "dy_nms_rotated", extra, &q.n);
  if (rc0 != DY_OK) return rc0;
  q.theta = theta;
  q.table = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(d->workspace) + rnms_table_offset(d->batch, d->anchors));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rcf = nms_launch_filter(q.n, d->prefiltered != 0, st);
  if (rcf != DY_OK) return rcf;
  hipLaunchKernelGGL(nms_rotated_kernel, dim3((unsigned)d->batch), dim3(RNMS_THREADS), 0, st, q);
  return check_launch("nms_rotated_kernel");
}

extern "C" int64_t dy_nms_rotated_ml_workspace_bytes(int32_t batch, int32_t anchors, int32_t nc) {
  if (batch <= 0 || anchors <= 0 || nc <= 0 || (long long)anchors * nc >= (1ll << 30)) return -1;
  const int cap = anchors * nc;
  return (int64_t)(rnms_table_offset(batch, cap) + (size_t)batch * 5 * (size_t)cap * 4);
}

extern "C" int32_t dy_nms_rotated_ml(const dy_nms_desc* d, const float* theta, dy_stream_t stream) {
  DY_REQUIRE(d && theta, DY_ERR_INVALID_ARG, "dy_nms_rotated_ml: null pointer");
  DY_REQUIRE(d->prefiltered == 0, DY_ERR_UNSUPPORTED, "dy_nms_rotated_ml: the fused candidate filter is single-label; multi_label filters here");
  dy_nms_desc m = *d;
  m.multi_label = 1;  // whatever the field says (nms_args_from_desc drops it again for nc == 1, ops.py:255)
  RNmsArgs q{};
  const bool dims = m.batch > 0 && m.anchors > 0 && m.nc > 0 && (long long)m.anchors * m.nc < (1ll << 30);
  const int cap = dims ? m.anchors * m.nc : 0;
  const int64_t extra = dims ? dy_nms_rotated_ml_workspace_bytes(m.batch, m.anchors, m.nc) - (int64_t)nms_ws_bytes(m.batch, cap) : 0;
  const int rc0 = nms_args_from_desc(&m, "dy_nms_rotated_ml", extra, &q.n);
  if (rc0 != DY_OK) return rc0;
  q.theta = theta;
  q.table = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(m.workspace) + rnms_table_offset(m.batch, q.n.cap));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rcf = nms_launch_filter(q.n, false, st);
  if (rcf != DY_OK) return rcf;
  if (q.n.multi) {
    hipLaunchKernelGGL(nms_rotated_ml_kernel, dim3((unsigned)m.batch), dim3(RNMS_THREADS), 0, st, q);
    return check_launch("nms_rotated_ml_kernel");
  }
  hipLaunchKernelGGL(nms_rotated_kernel, dim3((unsigned)m.batch), dim3(RNMS_THREADS), 0, st, q);  // nc == 1: single-label
  return check_launch("nms_rotated_kernel");
}

extern "C" int32_t dy_nms_rotated_lds_cap(void) { return RNMS_LDS_CAP; }

extern "C" int32_t dy_scale_rboxes(float* rows, const int32_t* counts, const float* params, int32_t batch, int32_t max_det,
                                   dy_stream_t stream) {
  DY_REQUIRE(rows && counts && params, DY_ERR_INVALID_ARG, "dy_scale_rboxes: null pointer");
  DY_REQUIRE(batch > 0 && max_det > 0 && (long long)batch * max_det < (1ll << 31), DY_ERR_INVALID_ARG, "dy_scale_rboxes: bad dims");
  const int total = batch * max_det;
  hipLaunchKernelGGL(scale_rboxes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rows,
                     counts, params, batch, max_det);
  return check_launch("scale_rboxes_kernel");
}
