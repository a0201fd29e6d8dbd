// ByteTrack on the padded dy_nms output: BYTETracker.update (trackers/byte_tracker.py:293-405) with STrack, KalmanFilterXYAH
// (trackers/utils/kalman_filter.py:65-236), iou_distance / fuse_score / linear_assignment (trackers/utils/matching.py) and the
// per-image rules of trackers/track.py:71-88, for S independent video streams and F time steps in ONE launch, no host in between.
//
//   track_step_kernel   one workgroup (256 threads) per stream; it walks its F images (image k = stream k % S at step k / S) in order.
//
// The tracks of a stream are a struct of arrays over max_tracks SLOTS (tracked, lost and unconfirmed together).  The reference's lists
// follow from the slot fields: tracked_stracks = state TRACKED (`act` tells confirmed from unconfirmed); lost_stracks = state LOST or
// REMOVED (a slot is freed the moment it leaves that list); of removed_stracks only membership by id matters = the slot's `inrem` flag.
// mean[8] / covariance[8x8] stay in device memory in float64 ([component][slot], so that neighbouring threads read neighbouring
// addresses) and are touched by one thread per slot; the small fields (state, id, score, ...) sit in LDS for the launch.
//
// Per image: detections -> float32 xyxy / xyah as STrack holds them; multi_predict of the pool; three linear assignments (pool x high
// scores at match_thresh with fuse_score, the still-TRACKED rest x low scores at 0.5, unconfirmed x remaining high scores at 0.7), each
// followed by the Kalman updates of its matches (4x4 Cholesky solve, one thread per match); new tracks (ids by ascending detection index);
// time-outs; remove_duplicate_stracks (IoU distance < 0.15, the younger one goes); the activated TRACKED slots out in ascending id.
//
// Linear assignment: lapjv(extend_cost, cost_limit = t) picks the matching that minimises the sum of (c - t) over matched pairs; a pair
// with c >= t (or NaN) is no edge.  Solved EXACTLY by successive shortest augmenting paths (the Hungarian method row by row, potentials
// in float64) on the rectangular problem rows x (columns + one private zero-cost dummy per row): a row ends on a column or on its dummy
// (= unmatched).  One wave runs it: the columns are spread over the 64 lanes, a Dijkstra step is one relaxation of the current row's
// edges, a wave-wide argmin and the potential update.  The costs are NOT stored: an edge's IoU is recomputed from the two boxes in LDS
// whenever a row is scanned (20 flops), so nothing is sized rows x columns.  Worst case: rows x (min(rows, columns) + 1) Dijkstra steps
// (512 x 301 at the defaults), each ceil(columns / 64) edges per lane + 6 shuffles; every loop is bounded by a count.
//
// The IoU follows bbox_ioa (utils/metrics.py:20-49) operation by operation in fp32 with contraction off and the correctly rounded
// division; a NaN anywhere in a box makes the cost NaN = no edge.
//
// Two instantiations of the one kernel over a box policy (as dy_val_match / dy_val_match_rotated): TkAxis above, and TkRot for the rows
// of an oriented-box model (trackers/track.py:69-88 `is_obb`, byte_tracker.py:68-79 / :217-228).  The Kalman filter, the solver, the
// compaction, the state machine and the output stage are shared; the policy changes the detection load ([x, y, w, h, r, conf, cls]: centre
// and size straight from the row), the record a cost is computed from (probiou.h's RRow: the covariance terms are computed once per slot
// and once per detection per image, one cosf / sinf pair per box, never per edge), the pair cost (1 - rnms_probiou(track, detection), then
// fuse_score) and the output row (xywh of the mean, the angle, id, score, cls, idx).  The angle is not filtered: a slot holds the fp32
// angle of the detection it last matched.
#include "common_hip.h"
#include "probiou.h"

#pragma clang fp contract(off)

namespace dy {

constexpr int TK_THREADS = 256;
constexpr int TK_MAX = 1024;  // bound of max_tracks and max_det (LDS per slot / per detection below)
constexpr int TK_HDR = 64;    // bytes in front of a stream's state: frame counter, id counter, overflow counter
constexpr int TK_FREE = 0, TK_TRACKED = 1, TK_LOST = 2, TK_REMOVED = 3;  // TrackState (basetrack.py:25-28); New = a free slot
constexpr int TK_SLOT_INTS = 9;                                           // state, act, m32, inrem, id, idx, frame_id, start_frame, tracklet_len
constexpr int TK_LDS_SLOT = 8 + 16 + (TK_SLOT_INTS + 2 + 2 + 3 + 1) * 4;  // u | tbox | fields, score, cls, waslost, dup, three lists, rmatch
constexpr int TK_LDS_DET = 16 + 16 + (1 + 1 + 1 + 3 + 3) * 4;             // v, minv | dbox | score, kind, used, three lists, way / cmatch / taken


// The box policies.  IN / OUT: floats of a detection row and of an output row; CONF / CLS: columns of a detection row; STATE_FLT: fp32
// fields of a slot in the device state (score, cls[, angle]); SLOT_WORDS / DET_WORDS: 4-byte LDS words a slot / a detection needs beyond
// the axis-aligned layout.  Rec is what a cost is computed from; the 16-byte part of it stays in the float4 arrays tbox / dbox, the fifth
// float of an RRow in arrays of its own, so that every 16-byte access is 16-byte aligned for every even max_tracks.
struct TkBoxes {
  float4* q;  // axis-aligned: xyxy; rotated: x, y and the covariance terms a, b
  float* c;   // rotated: the covariance term c
};
struct TkAxis {
  static constexpr bool ROT = false;
  static constexpr int IN = 6, OUT = 8, CONF = 4, CLS = 5, STATE_FLT = 2, SLOT_WORDS = 0, DET_WORDS = 0;
  using Rec = float4;
  static __device__ __forceinline__ Rec load(const TkBoxes& b, const int i) { return b.q[i]; }
};
struct TkRot {
  static constexpr bool ROT = true;
  static constexpr int IN = 7, OUT = 9, CONF = 5, CLS = 6, STATE_FLT = 3, SLOT_WORDS = 2, DET_WORDS = 1;  // slot: c, angle; detection: c
  using Rec = RRow;
  static __device__ __forceinline__ Rec load(const TkBoxes& b, const int i) {
    const float4 q = b.q[i];
    return RRow{q.x, q.y, q.z, q.w, b.c[i]};
  }
  static __device__ __forceinline__ void store(const TkBoxes& b, const int i, const RRow& r) {
    b.q[i] = make_float4(r.x, r.y, r.a, r.b);
    b.c[i] = r.c;
  }
};

template <typename Pol> static inline size_t track_state_bytes1(int max_tracks) {
  return (size_t)TK_HDR + (size_t)max_tracks * (72 * 8 + (TK_SLOT_INTS + Pol::STATE_FLT) * 4);  // a multiple of 8 for even max_tracks
}
static inline size_t track_ws_bytes1(int max_det) { return ((size_t)max_det * 16 + 255) / 256 * 256; }  // the xyah measurements of one image
template <typename Pol> static inline size_t track_lds_bytes(int max_tracks, int max_det) {
  return (size_t)max_tracks * (TK_LDS_SLOT + 4 * Pol::SLOT_WORDS) + (size_t)max_det * (TK_LDS_DET + 4 * Pol::DET_WORDS) + 64;
}

struct TrackArgs {
  const float* rows;
  const int* counts;
  unsigned char* state;
  unsigned char* ws;
  float* out;
  int* out_count;
  int frames, streams, max_det, max_tracks;
  float high, low, newt, match;
  int fuse, max_time_lost;
  long long state_stride, ws_stride;
};

// 1 - bbox_ioa(a, b, iou=True) [then fuse_score]: all fp32, in the reference's order of operations
__device__ __forceinline__ float tk_cost(const float4 a, const float4 b, const float score, const bool fuse) {
  const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = iw * ih;
  const float area_b = (b.z - b.x) * (b.w - b.y);
  const float area_a = (a.z - a.x) * (a.w - a.y);
  const float uni = (area_b + area_a) - inter;
  float cost = 1.f - __fdiv_rn(inter, uni + 1e-7f);
  if (fuse) cost = 1.f - (1.f - cost) * score;
  return cost;
}

// 1 - batch_probiou(track, detection) [then fuse_score] (matching.py:85-101): probiou.h's expression, arguments in the reference's order
__device__ __forceinline__ float tk_cost(const RRow& a, const RRow& b, const float score, const bool fuse) {
  float cost = 1.f - rnms_probiou(a, b);
  if (fuse) cost = 1.f - (1.f - cost) * score;
  return cost;
}

// STrack.xywh (byte_tracker.py:185-214) rounded to fp32: tlwh from the mean, then the centre back from the corner -- (x - w / 2) + w / 2
// is not always x, so the order stays; fp32 arithmetic while the mean is still initiate's float32 one
__device__ __forceinline__ float4 tk_xywh(const double x, const double y, const double a, const double h, const int m32) {
  if (m32) {
    const float hf = (float)h, w = (float)a * hf;
    const float x1 = (float)x - w / 2.f, y1 = (float)y - hf / 2.f;
    return make_float4(x1 + w / 2.f, y1 + hf / 2.f, w, hf);
  }
  const double w = a * h;
  const double x1 = x - w / 2.0, y1 = y - h / 2.0;
  return make_float4((float)(x1 + w / 2.0), (float)(y1 + h / 2.0), (float)w, (float)h);
}

// STrack.xyxy rounded to fp32; fp32 arithmetic while the mean is still initiate's float32 one
__device__ __forceinline__ float4 tk_xyxy(const double x, const double y, const double a, const double h, const int m32) {
  if (m32) {
    const float hf = (float)h, w = (float)a * hf;
    const float x1 = (float)x - w / 2.f, y1 = (float)y - hf / 2.f;
    return make_float4(x1, y1, w + x1, hf + y1);
  }
  const double w = a * h;
  const double x1 = x - w / 2.0, y1 = y - h / 2.0;
  return make_float4((float)x1, (float)y1, (float)(w + x1), (float)(h + y1));
}

// ordered compaction by ONE wave: out[] = the i in [0, n) with pred(i), ascending; returns their number (the same on every lane)
template <typename Pred> __device__ __forceinline__ int tk_compact(const int n, int* out, const int lane, Pred pred) {
  int cnt = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool p = i < n && pred(i);
    const unsigned long long m = __ballot(p);
    if (p) out[cnt + __popcll(m & ((1ull << lane) - 1ull))] = i;
    cnt += __popcll(m);
  }
  return cnt;
}

// LDS of the assignment.  One wave works on it in lockstep and lanes read what other lanes wrote: the LDS serves a wave's accesses in
// program order, and __builtin_amdgcn_wave_barrier() (no instruction) keeps the compiler from moving or caching accesses across the
// points where the ownership changes.
struct TkSolver {
  double* u;     // [rows] row potentials
  double* v;     // [cols] column potentials
  double* minv;  // [cols] shortest reduced distance found so far
  int* rmatch;   // [rows] column of the row, -1 = its dummy
  int* cmatch;   // [cols] row of the column, -1 = free
  int* way;      // [cols] the column in front on the shortest path, -1 = the start row
  int* taken;    // [cols] in the tree of this augmentation
};

// rows = slots rl[0..nr), columns = detections cl[0..nc); on return rmatch[r] = position in cl or -1.  Run by one whole wave.
template <typename Pol>
__device__ __forceinline__ void tk_assign(const TkSolver& s, const int* rl, const int nr, const int* cl, const int nc, const TkBoxes& tbox, const TkBoxes& dbox,
                          const float* dscore, const float thresh, const bool fuse, const int lane) {
  const double inf = __builtin_huge_val();
  const double t64 = (double)thresh;
  for (int j = lane; j < nc; j += 64) {
    s.v[j] = 0.0;
    s.cmatch[j] = -1;
  }
  for (int r = lane; r < nr; r += 64) {
    s.u[r] = 0.0;
    s.rmatch[r] = -1;
  }
  if (nc == 0) return;
  __builtin_amdgcn_wave_barrier();
  for (int i = 0; i < nr; ++i) {
    for (int j = lane; j < nc; j += 64) {
      s.minv[j] = inf;
      s.taken[j] = 0;
      s.way[j] = -1;
    }
    double dmin = inf;  // the cheapest way out through a dummy: reduced cost 0 - u[row] of a row of the tree
    int drow = -1;
    int cur = i, curcol = -1;
    for (int it = 0; it <= nc; ++it) {  // every step ends the augmentation or takes one more column into the tree
      __builtin_amdgcn_wave_barrier();
      const typename Pol::Rec a = Pol::load(tbox, rl[cur]);
      const double ucur = s.u[cur];
      if (-ucur < dmin) {
        dmin = -ucur;
        drow = cur;
      }
      double best = inf;
      int bestj = 0x7fffffff;
      for (int j = lane; j < nc; j += 64) {
        if (s.taken[j]) continue;
        const int d = cl[j];
        const float c = tk_cost(a, Pol::load(dbox, d), dscore[d], fuse);
        double mv = s.minv[j];
        if (c < thresh) {  // (false for NaN: no edge)
          const double red = (((double)c - t64) - ucur) - s.v[j];
          if (red < mv) {
            mv = red;
            s.minv[j] = red;
            s.way[j] = curcol;
          }
        }
        if (mv < best) {  // ascending j on a lane: the first of equal values stays
          best = mv;
          bestj = j;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oj = __shfl_xor(bestj, o);
        if (ob < best || (ob == best && oj < bestj)) {
          best = ob;
          bestj = oj;
        }
      }
      const bool to_dummy = !(best < dmin);  // dmin is finite (potentials are): an augmentation always ends
      const double delta = to_dummy ? dmin : best;
      // every row of the tree gains delta, every column of the tree loses it; the others come closer by it
      s.u[i] = s.u[i] + delta;  // (all lanes store the same value)
      for (int j = lane; j < nc; j += 64) {
        if (s.taken[j]) {
          const int r = s.cmatch[j];
          s.u[r] = s.u[r] + delta;
          s.v[j] = s.v[j] - delta;
        } else {
          s.minv[j] = s.minv[j] - delta;
        }
      }
      dmin -= delta;
      __builtin_amdgcn_wave_barrier();
      int j1;
      if (to_dummy) {
        if (drow == i) break;  // the new row stays unmatched
        j1 = s.rmatch[drow];   // drow moves to its dummy and hands its column back along the path
        s.rmatch[drow] = -1;
      } else {
        j1 = bestj;
        const int r = s.cmatch[j1];
        if (r >= 0) {  // taken by another row: that row joins the tree
          s.taken[j1] = 1;
          cur = r;
          curcol = j1;
          continue;
        }
      }
      for (int k = 0; k <= nc && j1 >= 0; ++k) {  // unwind: every column on the path goes to the row that reached it (all lanes alike)
        const int j0 = s.way[j1];
        const int r = j0 < 0 ? i : s.cmatch[j0];
        s.cmatch[j1] = r;
        s.rmatch[r] = j1;
        j1 = j0;
      }
      break;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// KalmanFilterXYAH.update of one slot with the fp32 measurement z (x, y, a, h); one thread
__device__ void tk_kalman_update(double* mean, double* cov, const int T, const int slot, const float4 z, const int m32) {
  double m[8], P[8][8];
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = mean[(size_t)k * T + slot];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) P[a][b] = cov[(size_t)(a * 8 + b) * T + slot];
  const double sd = m32 ? (double)((float)(1.0 / 20) * (float)m[3]) : (1.0 / 20) * m[3];
  double S[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) S[a][b] = P[a][b];
  S[0][0] += sd * sd;
  S[1][1] += sd * sd;
  S[2][2] += 1e-1 * 1e-1;
  S[3][3] += sd * sd;
  double L[4][4];  // S = L L^T
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      double acc = S[a][b];
#pragma unroll
      for (int k = 0; k < b; ++k) acc -= L[a][k] * L[b][k];
      L[a][b] = (a == b) ? sqrt(acc) : acc / L[b][b];
    }
  }
  double X[4][8];  // K^T = S^-1 (P H^T)^T
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    double y[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double acc = P[c][a];
#pragma unroll
      for (int k = 0; k < a; ++k) acc -= L[a][k] * y[k];
      y[a] = acc / L[a][a];
    }
#pragma unroll
    for (int a = 3; a >= 0; --a) {
      double acc = y[a];
#pragma unroll
      for (int k = a + 1; k < 4; ++k) acc -= L[k][a] * X[k][c];
      X[a][c] = acc / L[a][a];
    }
  }
  const double innov[4] = {(double)z.x - m[0], (double)z.y - m[1], (double)z.z - m[2], (double)z.w - m[3]};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) acc += innov[a] * X[a][c];
    mean[(size_t)c * T + slot] = m[c] + acc;
  }
  double M[4][8];  // S K^T
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += S[a][k] * X[k][c];
      M[a][c] = acc;
    }
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += X[k][a] * M[k][b];
      cov[(size_t)(a * 8 + b) * T + slot] = P[a][b] - acc;
    }
}

template <typename Pol> __global__ __launch_bounds__(TK_THREADS) void track_step_kernel(const TrackArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  const int T = p.max_tracks, D = p.max_det;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sidx_stream = blockIdx.x;
  // ---- LDS carve: 8-byte items first ----
  double* s_u = reinterpret_cast<double*>(dyn_smem);  // [T]
  double* s_v = s_u + T;                               // [D]
  double* s_minv = s_v + D;                            // [D]
  float4* tbox4 = reinterpret_cast<float4*>(s_minv + D);  // [T] every slot's box as iou_distance sees it (T * 8 + D * 16 bytes in front: 16-byte aligned for even T)
  float4* dbox4 = tbox4 + T;                              // [D]
  int* sst = reinterpret_cast<int*>(dbox4 + D);           // [T] each of the following
  int* sact = sst + T;
  int* sm32 = sact + T;
  int* sinrem = sm32 + T;
  int* sid = sinrem + T;
  int* sdi = sid + T;  // detection index of the last match
  int* sfid = sdi + T;
  int* sstart = sfid + T;
  int* stlen = sstart + T;
  float* sscore = reinterpret_cast<float*>(stlen + T);
  float* scls = sscore + T;
  int* swl = reinterpret_cast<int*>(scls + T);  // in the lost list when the update began
  int* sdup = swl + T;
  int* listA = sdup + T;
  int* listB = listA + T;
  int* listC = listB + T;
  int* s_rmatch = listC + T;
  float* trc = reinterpret_cast<float*>(s_rmatch + T);  // rotated only ([T] each; no bytes otherwise): the fifth float of a slot's RRow,
  float* sang = trc + (Pol::ROT ? T : 0);                 // and the angle of the detection the slot last matched
  float* dscore = sang + (Pol::ROT ? T : 0);              // [D] each of the following
  int* dkind = reinterpret_cast<int*>(dscore + D);
  int* dused = dkind + D;
  int* clH = dused + D;
  int* clL = clH + D;
  int* clR = clL + D;
  int* s_way = clR + D;
  int* s_cmatch = s_way + D;
  int* s_taken = s_cmatch + D;
  float* drc = reinterpret_cast<float*>(s_taken + D);            // rotated only ([D]): the fifth float of a detection's RRow
  int* s_n = reinterpret_cast<int*>(drc + (Pol::ROT ? D : 0));     // [16] list lengths
  const TkBoxes tbox{tbox4, trc}, dbox{dbox4, drc};
  TkSolver sol{s_u, s_v, s_minv, s_rmatch, s_cmatch, s_way, s_taken};

  unsigned char* sbase = p.state + (size_t)sidx_stream * p.state_stride;
  int* hdr = reinterpret_cast<int*>(sbase);
  double* mean = reinterpret_cast<double*>(sbase + TK_HDR);  // [8][T]
  double* cov = mean + (size_t)8 * T;                        // [64][T]
  int* gint = reinterpret_cast<int*>(cov + (size_t)64 * T);  // [TK_SLOT_INTS][T]
  float* gflt = reinterpret_cast<float*>(gint + (size_t)TK_SLOT_INTS * T);  // [Pol::STATE_FLT][T]
  float4* dxyah = reinterpret_cast<float4*>(p.ws + (size_t)sidx_stream * p.ws_stride);  // [D] the measurements of the image at hand

  for (int s = tid; s < T; s += TK_THREADS) {
    sst[s] = gint[s];
    sact[s] = gint[T + s];
    sm32[s] = gint[2 * T + s];
    sinrem[s] = gint[3 * T + s];
    sid[s] = gint[4 * T + s];
    sdi[s] = gint[5 * T + s];
    sfid[s] = gint[6 * T + s];
    sstart[s] = gint[7 * T + s];
    stlen[s] = gint[8 * T + s];
    sscore[s] = gflt[s];
    scls[s] = gflt[T + s];
    if constexpr (Pol::ROT) sang[s] = gflt[2 * T + s];
  }
  int frame = hdr[0], next_id = hdr[1], overflow = hdr[2];  // the same on every thread throughout
  __syncthreads();

  // a slot's box for the costs, from its mean (and, rotated, the angle it holds): after every change of the mean or the angle
  auto put_box = [&](const int s, const double x, const double y, const double a, const double h, const int m32) {
    if constexpr (Pol::ROT) {
      const float4 b = tk_xywh(x, y, a, h, m32);
      Pol::store(tbox, s, rnms_row(b.x, b.y, b.z, b.w, sang[s]));
    } else {
      tbox4[s] = tk_xyxy(x, y, a, h, m32);
    }
  };

  for (int f = 0; f < p.frames; ++f) {
    const int img = f * p.streams + sidx_stream;
    int n = p.counts[img];
    n = n < 0 ? 0 : (n > D ? D : n);
    float* orow = p.out + (size_t)img * T * Pol::OUT;
    if (n == 0) {  // trackers/track.py:79-80: the image does not reach the tracker (uniform branch)
      for (int i = tid; i < T * Pol::OUT; i += TK_THREADS) orow[i] = 0.f;
      if (tid == 0) p.out_count[img] = 0;
      continue;
    }
    ++frame;
    const float* rb = p.rows + (size_t)img * D * Pol::IN;
    // ---- detections as STrack holds them; multi_predict of the pool; every slot's box ----
    for (int d = tid; d < n; d += TK_THREADS) {
      const float* r = rb + (size_t)d * Pol::IN;
      const float conf = r[Pol::CONF];
      float cx, cy, w, h;
      if constexpr (Pol::ROT) {
        cx = r[0], cy = r[1], w = r[2], h = r[3];  // OBB.xywhr: centre and size straight from the row
      } else {
        const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
        cx = (x1 + x2) / 2.f, cy = (y1 + y2) / 2.f, w = x2 - x1, h = y2 - y1;  // Boxes.xywh (ops.xyxy2xywh) in fp32
      }
      const float lx = (float)((double)cx - (double)w / 2.0), ly = (float)((double)cy - (double)h / 2.0);  // xywh2ltwh on the float64 row, stored as fp32
      const float4 z = make_float4(lx + w / 2.f, ly + h / 2.f, __fdiv_rn(w, h), h);
      if constexpr (Pol::ROT) Pol::store(dbox, d, rnms_row(z.x, z.y, w, h, r[4]));  // STrack.xywha of a detection: _tlwh.xy + _tlwh.wh / 2, w, h, angle
      else dbox4[d] = make_float4(lx, ly, w + lx, h + ly);
      dxyah[d] = z;
      dscore[d] = conf;
      dkind[d] = conf >= p.high ? 1 : ((conf > p.low && conf < p.high) ? 2 : 0);
      dused[d] = 0;
    }
    for (int s = tid; s < T; s += TK_THREADS) {
      const int st = sst[s];
      sdup[s] = 0;
      swl[s] = 0;
      if (st == TK_FREE) continue;
      const bool inpool = (st == TK_TRACKED && sact[s]) || st == TK_LOST || st == TK_REMOVED;
      double m[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) m[k] = mean[(size_t)k * T + s];
      if (inpool) {
        swl[s] = st != TK_TRACKED;
        if (st != TK_TRACKED) m[7] = 0.0;
        const double sp = (1.0 / 20) * m[3], sv = (1.0 / 160) * m[3];
        const double q[8] = {sp * sp, sp * sp, 1e-2 * 1e-2, sp * sp, sv * sv, sv * sv, 1e-5 * 1e-5, sv * sv};
        double P[8][8];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) P[a][b] = cov[(size_t)(a * 8 + b) * T + s];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) P[a][b] = P[a][b] + P[a + 4][b];  // F P
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) P[a][b] = P[a][b] + P[a][b + 4];  // (F P) F^T
#pragma unroll
        for (int a = 0; a < 8; ++a) P[a][a] += q[a];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) cov[(size_t)(a * 8 + b) * T + s] = P[a][b];
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = m[k] + m[k + 4];
#pragma unroll
        for (int k = 0; k < 8; ++k) mean[(size_t)k * T + s] = m[k];
        sm32[s] = 0;
      }
      put_box(s, m[0], m[1], m[2], m[3], sm32[s]);
    }
    __syncthreads();
    // ---- the lists of the first association ----
    if (wave == 0) {
      const int c = tk_compact(T, listA, lane, [&](int s) { return sst[s] != TK_FREE && ((sst[s] == TK_TRACKED && sact[s]) || sst[s] == TK_LOST || sst[s] == TK_REMOVED); });
      if (lane == 0) s_n[0] = c;
    } else if (wave == 1) {
      const int c = tk_compact(n, clH, lane, [&](int d) { return dkind[d] == 1; });
      if (lane == 0) s_n[1] = c;
    } else if (wave == 2) {
      const int c = tk_compact(n, clL, lane, [&](int d) { return dkind[d] == 2; });
      if (lane == 0) s_n[2] = c;
    } else {
      const int c = tk_compact(T, listC, lane, [&](int s) { return sst[s] == TK_TRACKED && !sact[s]; });  // unconfirmed (no new track exists yet)
      if (lane == 0) s_n[3] = c;
    }
    __syncthreads();
    const int nA = s_n[0], nH = s_n[1], nL = s_n[2], nC = s_n[3];
    if (wave == 0) tk_assign<Pol>(sol, listA, nA, clH, nH, tbox, dbox, dscore, p.match, p.fuse != 0, lane);
    __syncthreads();
    // ---- matches of a list: STrack.update (tracked) / re_activate (lost); one thread per row ----
    auto apply = [&](const int* rl, const int nr, const int* cl, const bool mark) {
      for (int r = tid; r < nr; r += TK_THREADS) {
        const int c = s_rmatch[r];
        if (c < 0) continue;
        const int s = rl[r], d = cl[c];
        tk_kalman_update(mean, cov, T, s, dxyah[d], sm32[s]);
        sm32[s] = 0;
        stlen[s] = sst[s] == TK_TRACKED ? stlen[s] + 1 : 0;
        sst[s] = TK_TRACKED;
        sact[s] = 1;
        sfid[s] = frame;
        sscore[s] = dscore[d];
        scls[s] = rb[(size_t)d * Pol::IN + Pol::CLS];
        if constexpr (Pol::ROT) sang[s] = rb[(size_t)d * Pol::IN + 4];
        sdi[s] = d;
        if (mark) dused[d] = 1;
        put_box(s, mean[s], mean[(size_t)T + s], mean[(size_t)2 * T + s], mean[(size_t)3 * T + s], 0);
      }
    };
    apply(listA, nA, clH, true);
    __syncthreads();
    // ---- second association: what is left of the TRACKED pool against the low scores; the high scores still free for the unconfirmed ----
    if (wave == 0) {
      int cnt = 0;  // ordered compaction of listA's unmatched TRACKED rows into listB (slots)
      for (int base = 0; base < nA; base += 64) {
        const int r = base + lane;
        const bool ok = r < nA && s_rmatch[r] < 0 && sst[listA[r]] == TK_TRACKED;
        const unsigned long long m = __ballot(ok);
        if (ok) listB[cnt + __popcll(m & ((1ull << lane) - 1ull))] = listA[r];
        cnt += __popcll(m);
      }
      if (lane == 0) s_n[4] = cnt;
    } else if (wave == 1) {
      int cnt = 0;
      for (int base = 0; base < nH; base += 64) {
        const int c = base + lane;
        const bool ok = c < nH && !dused[clH[c]];
        const unsigned long long m = __ballot(ok);
        if (ok) clR[cnt + __popcll(m & ((1ull << lane) - 1ull))] = clH[c];
        cnt += __popcll(m);
      }
      if (lane == 0) s_n[5] = cnt;
    }
    __syncthreads();
    const int nB = s_n[4], nR = s_n[5];
    if (wave == 0) tk_assign<Pol>(sol, listB, nB, clL, nL, tbox, dbox, dscore, 0.5f, false, lane);
    __syncthreads();
    apply(listB, nB, clL, false);
    for (int r = tid; r < nB; r += TK_THREADS)
      if (s_rmatch[r] < 0) sst[listB[r]] = TK_LOST;  // mark_lost
    __syncthreads();
    // ---- unconfirmed tracks ----
    if (wave == 0) tk_assign<Pol>(sol, listC, nC, clR, nR, tbox, dbox, dscore, 0.7f, p.fuse != 0, lane);
    __syncthreads();
    apply(listC, nC, clR, true);
    for (int r = tid; r < nC; r += TK_THREADS)
      if (s_rmatch[r] < 0) sst[listC[r]] = TK_FREE;  // removed, and in no list
    __syncthreads();
    // ---- new tracks: the free high scores at or above new_track_thresh, ascending; the free slots, ascending ----
    if (wave == 0) {
      int cnt = 0;
      for (int base = 0; base < nR; base += 64) {
        const int c = base + lane;
        const bool ok = c < nR && !dused[clR[c]] && !(dscore[clR[c]] < p.newt);
        const unsigned long long m = __ballot(ok);
        if (ok) clL[cnt + __popcll(m & ((1ull << lane) - 1ull))] = clR[c];
        cnt += __popcll(m);
      }
      if (lane == 0) s_n[6] = cnt;
    } else if (wave == 1) {
      const int c = tk_compact(T, listA, lane, [&](int s) { return sst[s] == TK_FREE; });
      if (lane == 0) s_n[7] = c;
    }
    __syncthreads();
    {
      const int nN = s_n[6], nF = s_n[7];
      const int nk = nN < nF ? nN : nF;
      for (int k = tid; k < nk; k += TK_THREADS) {  // STrack.activate: KalmanFilterXYAH.initiate
        const int s = listA[k], d = clL[k];
        const float4 z = dxyah[d];
        const double sp = (double)((float)(2 * (1.0 / 20)) * z.w), sv = (double)((float)(10 * (1.0 / 160)) * z.w);  // fp32 products (numpy's scalar rule)
        const double q[8] = {sp * sp, sp * sp, 1e-2 * 1e-2, sp * sp, sv * sv, sv * sv, 1e-5 * 1e-5, sv * sv};
        const double m[8] = {(double)z.x, (double)z.y, (double)z.z, (double)z.w, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 8; ++a) mean[(size_t)a * T + s] = m[a];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) cov[(size_t)(a * 8 + b) * T + s] = a == b ? q[a] : 0.0;
        sst[s] = TK_TRACKED;
        sact[s] = frame == 1;
        sm32[s] = 1;
        sinrem[s] = 0;
        sid[s] = next_id + 1 + k;
        sdi[s] = d;
        sfid[s] = frame;
        sstart[s] = frame;
        stlen[s] = 0;
        sscore[s] = dscore[d];
        scls[s] = rb[(size_t)d * Pol::IN + Pol::CLS];
        if constexpr (Pol::ROT) sang[s] = rb[(size_t)d * Pol::IN + 4];
        put_box(s, m[0], m[1], m[2], m[3], 1);
      }
      next_id += nk;
      overflow += nN - nk;
    }
    __syncthreads();
    // ---- time-outs of what was in the lost list when the update began; that list is filtered against the removals of EARLIER updates only ----
    for (int s = tid; s < T; s += TK_THREADS) {
      int st = sst[s];
      if (st == TK_FREE) continue;
      bool pend = false;
      if (swl[s] && st != TK_TRACKED && frame - sfid[s] > p.max_time_lost) {
        st = TK_REMOVED;
        pend = true;
      }
      if ((st == TK_LOST || st == TK_REMOVED) && sinrem[s]) st = TK_FREE;
      else if (pend) sinrem[s] = 1;  // appended after the filter: stays for one more update
      sst[s] = st;
    }
    __syncthreads();
    // ---- remove_duplicate_stracks ----
    if (wave == 0) {
      const int c = tk_compact(T, listA, lane, [&](int s) { return sst[s] == TK_TRACKED; });
      if (lane == 0) s_n[8] = c;
    } else if (wave == 1) {
      const int c = tk_compact(T, listB, lane, [&](int s) { return sst[s] == TK_LOST || sst[s] == TK_REMOVED; });
      if (lane == 0) s_n[9] = c;
    }
    __syncthreads();
    {
      const int nTa = s_n[8], nTb = s_n[9];
      for (int i = tid; i < nTa; i += TK_THREADS) {
        const int a = listA[i];
        const typename Pol::Rec ba = Pol::load(tbox, a);
        const int ta = sfid[a] - sstart[a];
        bool drop = false;
        for (int k = 0; k < nTb; ++k) {
          const int b = listB[k];
          if (tk_cost(ba, Pol::load(tbox, b), 0.f, false) < 0.15f) {
            if (ta > sfid[b] - sstart[b]) sdup[b] = 1;  // (several threads may store the same 1)
            else drop = true;
          }
        }
        if (drop) sdup[a] = 1;
      }
    }
    __syncthreads();
    for (int s = tid; s < T; s += TK_THREADS)
      if (sdup[s]) sst[s] = TK_FREE;
    __syncthreads();
    // ---- STrack.result of the activated TRACKED slots, in ascending id ----
    if (wave == 0) {
      const int c = tk_compact(T, listA, lane, [&](int s) { return sst[s] == TK_TRACKED && sact[s]; });
      if (lane == 0) s_n[10] = c;
    }
    __syncthreads();
    {
      const int nO = s_n[10];
      for (int i = tid; i < nO; i += TK_THREADS) {
        const int s = listA[i], id = sid[s];
        int rank = 0;
        for (int k = 0; k < nO; ++k) rank += sid[listA[k]] < id;  // ids are unique
        float* o = orow + (size_t)rank * Pol::OUT;
        float4 b;
        if constexpr (Pol::ROT) {  // STrack.xywha: the box from the mean as the costs saw it, and the angle held
          b = tk_xywh(mean[s], mean[(size_t)T + s], mean[(size_t)2 * T + s], mean[(size_t)3 * T + s], sm32[s]);
          o[4] = sang[s];
        } else {
          b = tbox4[s];
        }
        o[0] = b.x, o[1] = b.y, o[2] = b.z, o[3] = b.w;
        o[Pol::OUT - 4] = (float)id, o[Pol::OUT - 3] = sscore[s], o[Pol::OUT - 2] = scls[s], o[Pol::OUT - 1] = (float)sdi[s];
      }
      for (int i = nO * Pol::OUT + tid; i < T * Pol::OUT; i += TK_THREADS) orow[i] = 0.f;
      if (tid == 0) p.out_count[img] = nO;
    }
    __syncthreads();
  }

  for (int s = tid; s < T; s += TK_THREADS) {
    gint[s] = sst[s];
    gint[T + s] = sact[s];
    gint[2 * T + s] = sm32[s];
    gint[3 * T + s] = sinrem[s];
    gint[4 * T + s] = sid[s];
    gint[5 * T + s] = sdi[s];
    gint[6 * T + s] = sfid[s];
    gint[7 * T + s] = sstart[s];
    gint[8 * T + s] = stlen[s];
    gflt[s] = sscore[s];
    gflt[T + s] = scls[s];
    if constexpr (Pol::ROT) gflt[2 * T + s] = sang[s];
  }
  if (tid == 0) {
    hdr[0] = frame;
    hdr[1] = next_id;
    hdr[2] = overflow;
  }
}

}  // namespace dy

using namespace dy;

static bool track_dims_ok(int streams, int max_tracks, const char* who) {
  if (streams > 0 && max_tracks > 0 && max_tracks <= TK_MAX && max_tracks % 2 == 0) return true;
  set_error("%s: bad dims (streams %d, max_tracks %d; streams > 0, max_tracks even and in [2,%d])", who, streams, max_tracks, TK_MAX);
  return false;
}

// the entry points of a policy; `who` is the exported name
template <typename Pol> static int64_t track_state_bytes_t(int32_t streams, int32_t max_tracks, const char* who) {
  if (!track_dims_ok(streams, max_tracks, who)) return DY_ERR_INVALID_ARG;
  return (int64_t)streams * (int64_t)track_state_bytes1<Pol>(max_tracks);
}

static int64_t track_workspace_bytes_t(int32_t streams, int32_t max_tracks, int32_t max_det, const char* who) {
  if (!track_dims_ok(streams, max_tracks, who)) return DY_ERR_INVALID_ARG;
  if (max_det <= 0 || max_det > TK_MAX) {
    set_error("%s: max_det %d must be in [1,%d]", who, max_det, TK_MAX);
    return DY_ERR_INVALID_ARG;
  }
  return (int64_t)streams * (int64_t)track_ws_bytes1(max_det);
}

template <typename Pol> static int32_t track_reset_t(void* state, int32_t streams, int32_t max_tracks, dy_stream_t stream, const char* who) {
  DY_REQUIRE(state, DY_ERR_INVALID_ARG, "%s: null state pointer", who);
  if (!track_dims_ok(streams, max_tracks, who)) return DY_ERR_INVALID_ARG;
  zero_async(state, (size_t)streams * track_state_bytes1<Pol>(max_tracks), reinterpret_cast<hipStream_t>(stream));  // all slots free, counters 0
  return check_launch("zero_words_kernel");
}

template <typename Pol> static int32_t track_step_t(const dy_track_desc* d, dy_stream_t stream, const char* who, const char* kernel) {
  DY_REQUIRE(d && d->rows && d->counts && d->state && d->workspace && d->out && d->out_count, DY_ERR_INVALID_ARG,
             "%s: null pointer (rows / counts / state / workspace / out / out_count)", who);
  DY_REQUIRE(d->frames > 0 && d->streams > 0 && d->max_det > 0 && d->max_det <= TK_MAX, DY_ERR_INVALID_ARG,
             "%s: bad dims (frames %d, streams %d, max_det %d; all positive, max_det <= %d)", who, d->frames, d->streams, d->max_det, TK_MAX);
  if (!track_dims_ok(d->streams, d->max_tracks, who)) return DY_ERR_INVALID_ARG;
  DY_REQUIRE(d->max_time_lost >= 0, DY_ERR_INVALID_ARG, "%s: max_time_lost %d < 0", who, d->max_time_lost);
  const size_t lds = track_lds_bytes<Pol>(d->max_tracks, d->max_det);
  DY_REQUIRE(lds <= 160 * 1024, DY_ERR_INVALID_ARG, "%s: max_tracks %d with max_det %d needs %zu bytes of LDS (160 KB at most)", who, d->max_tracks,
             d->max_det, lds);
  DY_REQUIRE(d->state_bytes >= (int64_t)d->streams * (int64_t)track_state_bytes1<Pol>(d->max_tracks), DY_ERR_WORKSPACE,
             "%s: state of %lld bytes, dy_track_state_bytes%s asks for more", who, (long long)d->state_bytes, Pol::ROT ? "_rotated" : "");
  DY_REQUIRE(d->workspace_bytes >= (int64_t)d->streams * (int64_t)track_ws_bytes1(d->max_det), DY_ERR_WORKSPACE,
             "%s: workspace of %lld bytes, dy_track_workspace_bytes%s asks for more", who, (long long)d->workspace_bytes, Pol::ROT ? "_rotated" : "");
  DY_REQUIRE(((uintptr_t)d->state & 15) == 0 && ((uintptr_t)d->workspace & 15) == 0, DY_ERR_INVALID_ARG, "%s: state / workspace not 16-byte aligned", who);
  TrackArgs a{};
  a.rows = d->rows;
  a.counts = d->counts;
  a.state = reinterpret_cast<unsigned char*>(d->state);
  a.ws = reinterpret_cast<unsigned char*>(d->workspace);
  a.out = d->out;
  a.out_count = d->out_count;
  a.frames = d->frames;
  a.streams = d->streams;
  a.max_det = d->max_det;
  a.max_tracks = d->max_tracks;
  a.high = d->track_high_thresh;
  a.low = d->track_low_thresh;
  a.newt = d->new_track_thresh;
  a.match = d->match_thresh;
  a.fuse = d->fuse_score;
  a.max_time_lost = d->max_time_lost;
  a.state_stride = (long long)track_state_bytes1<Pol>(d->max_tracks);
  a.ws_stride = (long long)track_ws_bytes1(d->max_det);
  static const hipError_t attr_once = hipFuncSetAttribute((const void*)track_step_kernel<Pol>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  (void)attr_once;
  hipLaunchKernelGGL(track_step_kernel<Pol>, dim3((unsigned)d->streams), dim3(TK_THREADS), lds, reinterpret_cast<hipStream_t>(stream), a);
  return check_launch(kernel);
}

extern "C" int64_t dy_track_state_bytes(int32_t streams, int32_t max_tracks) { return track_state_bytes_t<TkAxis>(streams, max_tracks, "dy_track_state_bytes"); }
extern "C" int64_t dy_track_workspace_bytes(int32_t streams, int32_t max_tracks, int32_t max_det) {
  return track_workspace_bytes_t(streams, max_tracks, max_det, "dy_track_workspace_bytes");
}
extern "C" int32_t dy_track_reset(void* state, int32_t streams, int32_t max_tracks, dy_stream_t stream) {
  return track_reset_t<TkAxis>(state, streams, max_tracks, stream, "dy_track_reset");
}
extern "C" int32_t dy_track_step(const dy_track_desc* d, dy_stream_t stream) { return track_step_t<TkAxis>(d, stream, "dy_track_step", "track_step_kernel"); }

extern "C" int64_t dy_track_state_bytes_rotated(int32_t streams, int32_t max_tracks) {
  return track_state_bytes_t<TkRot>(streams, max_tracks, "dy_track_state_bytes_rotated");
}
extern "C" int64_t dy_track_workspace_bytes_rotated(int32_t streams, int32_t max_tracks, int32_t max_det) {
  return track_workspace_bytes_t(streams, max_tracks, max_det, "dy_track_workspace_bytes_rotated");
}
extern "C" int32_t dy_track_reset_rotated(void* state, int32_t streams, int32_t max_tracks, dy_stream_t stream) {
  return track_reset_t<TkRot>(state, streams, max_tracks, stream, "dy_track_reset_rotated");
}
extern "C" int32_t dy_track_step_rotated(const dy_track_desc* d, dy_stream_t stream) {
  return track_step_t<TkRot>(d, stream, "dy_track_step_rotated", "track_step_kernel<rotated>");
}
