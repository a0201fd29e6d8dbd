/*
 * dyolo.h — C-ABI of libdyolo.so, the MI355X (gfx950) device library for the
 * Drone-YOLO detection hot path.
 *
 * The reference (ultralytics fork, /root/reference) has no FFI boundary of its
 * own: its seam is Python nn.Modules looked up by name (nn/tasks.py:1012-1018)
 * that call torch ATen ops.  Every entry point below replaces the torch call
 * sites named in its comment; the Python host mirror (drone-yolo_amd/nn/...,
 * utils/ops.py) binds them with ctypes exactly as INTEGRATION.md shows.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types, no C++ types.
 *   - all pointers are DEVICE pointers unless a comment says "host".
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*),
 *     re-entrant, never allocates or frees, never synchronises.
 *   - return value: DY_OK (0) or a negative dy_status; the message for the
 *     last failure on the calling thread is dy_last_error_string().
 *   - activations are NHWC ("channels last"): element (n,h,w,c) of a view lives
 *     at base + ((n*H + h)*W + w)*ld + c, where ld >= C is the pixel pitch in
 *     ELEMENTS.  A channel slice of a wider buffer is therefore just another
 *     (base, ld) pair: Concat / chunk are done by construction, not by copies
 *     (reference: nn/modules/conv.py:323-333, block.py:237-242).
 *   - dtype of activations/weights: DY_BF16, DY_F16 or DY_F32.  Accumulation,
 *     bias, SiLU and residual adds are always fp32.
 */
#ifndef DYOLO_H_
#define DYOLO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYOLO_VERSION_MAJOR 0
#define DYOLO_VERSION_MINOR 1

typedef void* dy_stream_t; /* hipStream_t */

typedef enum dy_status {
  DY_OK = 0,
  DY_ERR_INVALID_ARG = -1,   /* null pointer, bad size, misaligned view */
  DY_ERR_UNSUPPORTED = -2,   /* shape / dtype combination not built */
  DY_ERR_LAUNCH = -3,        /* hipLaunchKernel / HIP runtime error */
  DY_ERR_WORKSPACE = -4      /* workspace too small */
} dy_status;

/* DY_FP8 = OCP e4m3fn (gfx950's fp8, NOT MI300's fnuz): 1 byte per element, 16 per 16-byte chunk.  An fp8 activation or weight
 * element q stands for the real value q * scale (dy_conv_desc.act_scale for activations, w_scale[co] / act_scale for the weights of
 * output channel co).  Entry points that are not built for it return DY_ERR_INVALID_ARG ("bad dtype"). */
typedef enum dy_dtype { DY_BF16 = 0, DY_F16 = 1, DY_F32 = 2, DY_FP8 = 3, DY_F16X2 = 4 } dy_dtype;
/* DY_F16X2 = SPLIT float16 storage (round 5): the bar-exact precision at 16-bit MFMA speed.  An element x is the pair
 *   hi = rn_f16(x) (0 when |x| < 2^-14),  lo = rn_f16((x - hi) * 2^11),      x ~= hi + lo * 2^-11   (22 mantissa bits)
 * and occupies 4 bytes like an fp32 element; within a pixel row every group of 8 channels is 32 bytes, the 8 hi halves then the 8 lo
 * halves ([hi c..c+7 | lo c..c+7]): a channel slice at a multiple of 8 channels is a contiguous byte range (Concat / chunk by view as
 * for the other types, pitches counted in 4-byte elements), and a 128-byte K-step of the implicit GEMM holds four (hi, lo) chunk
 * pairs, so one staged step feeds THREE v_mfma_f32_16x16x32_f16 per fragment pair — w_hi x_hi + w_lo x_hi + (w_hi 2^-11) x_lo, fp32
 * accumulate; the lo x lo term (2^-22 relative) is dropped.  Weights (DY_WLAYOUT_ROWS only) are packed the same way per (tap, 8
 * channels) after each output-channel row was scaled by a power of two into [2^13, 2^14) (w_lo unscaled); dy_conv_desc.w_scale[co]
 * holds the inverse power and multiplies the accumulator in the epilogue.  Built in dy_conv2d_nhwc (dense 1x1 / 3x3, stride 1 / 2,
 * residual, x2 / up2x, out_f32; and the GROUPED form of DWConv, conv.py:102-107 — cout == groups, 1 / 2 / 4 input channels per group,
 * cout % 8 == 0, plain call: there w is fp32 [cout][ksize * ksize * (cin / groups)], unscaled, no w_scale, and the kernel multiplies joined
 * fp32 inputs by it), dy_nchw_f32_to_nhwc, dy_nhwc_to_nchw_f32, dy_sppf_maxpool3 and the chunk copies; the reference has
 * no counterpart (its CPU path is fp32: this type reproduces it to ~4 fp32 ulps per layer, see tests/test_kernels_gpu.py). */
/* DY_ACT_SILU_L2E: SiLU in the log2(e)-SCALED activation domain.  The caller packs every bias multiplied by log2(e) (and the weights of a
 * layer that reads unscaled data, e.g. the image, likewise), so the accumulator holds t = log2(e) * z; the epilogue computes
 * t / (1 + 2^-t) = log2(e) * silu(z): every stored activation of the pass is log2(e) times the reference's (max pool, nearest upsample,
 * Concat and the Bottleneck sum commute with the positive scale) and the layers that leave the domain (the last 1x1 of each Detect
 * branch) carry weights divided by log2(e).  One VALU instruction less per output element than DY_ACT_SILU (sigmoid(z) = 1 / (1 + 2^-t)
 * needs no multiply in front of v_exp_f32).  The host mirror uses it for 16-bit / fp8 inference (drone-yolo_amd/hip_ops.py::scaled_activations). */
typedef enum dy_act { DY_ACT_NONE = 0, DY_ACT_SILU = 1, DY_ACT_SILU_L2E = 2 } dy_act;
/* Packed weight layouts of dy_conv2d_nhwc (see dy_conv_desc.w_layout). */
typedef enum dy_wlayout { DY_WLAYOUT_ROWS = 0, DY_WLAYOUT_HALO3X3 = 1, DY_WLAYOUT_FRAG1X1 = 2 } dy_wlayout;

/* ---- library -------------------------------------------------------------- */

/* (major << 16) | minor. */
int32_t dy_version(void);
/* Message of the last error raised on this thread ("" if none). Host string. */
const char* dy_last_error_string(void);
/* Introspection for measurement (bench.py's roofline.dominant_kernel): name of the device kernel the last launching call on this
 * thread dispatched to ("conv3x3_vgemm16_kernel", "conv_gemm_glds_kernel<256,256>", ...), so that live per-launch timings can be
 * grouped by the same symbols a rocprofv3 kernel trace reports.  Host string with static storage; "" before the first launch. */
const char* dy_last_kernel_name(void);
/* Size in bytes of one element of `dtype` (2, 2, 4, 1, 4) or 0 if unknown. */
int32_t dy_dtype_size(int32_t dtype);

/* ---- convolution ----------------------------------------------------------
 * Replaces: Conv.forward / forward_fuse = SiLU(BN(conv2d(x))) (nn/modules/conv.py:37-55),
 * RepVGGBlock.forward after get_equivalent_kernel_bias folding (nn/modules/block.py:1421-1490),
 * Bottleneck.forward's residual add (block.py:348-350), the plain nn.Conv2d 1x1 heads
 * of Detect (nn/modules/head.py:43-57) and DWConv (conv.py:102-107, groups > 1).
 *
 * y[n,ho,wo,co] = act( sum_{r,q,c} x[n, ho*stride - pad + r, wo*stride - pad + q, c]
 *                                   * w[co][(r*ksize + q)*cin + c]  + bias[co] ) (+ residual)
 *
 * Weights are PACKED by the caller:  row co holds the K = ksize*ksize*cin taps in
 * (r, q, c) order, rows are k_pad elements apart, k_pad = dy_conv_k_pad(...), rows
 * co >= cout up to cout_pad = dy_conv_cout_pad(cout) and columns k >= K must be ZERO.
 * BatchNorm (eps, running stats) and RepVGG branches are folded into w/bias by the
 * caller (utils/torch_utils.py:242-269 is the folding rule).
 * bias: fp32[cout_pad].  residual (optional, same dtype as x) is added AFTER the
 * activation.  Requirements: cin % (16/elem_size) == 0, ld_* and view bases aligned
 * to 16 bytes (vector path) — unaligned OUTPUT views fall back to scalar stores.
 *
 * Views.  x, x2, residual and y are VIEWS: channel slices of wider buffers (a Concat's input or output), pitches padded to 16 bytes
 * with whatever the allocation held.  Of a view a launch reads only elements [0, c) of the view's pixels and writes only elements
 * [0, cout) of the output's pixels, whatever the surrounding bytes hold: the channels in front of and behind the slice, the rest of
 * the pitch and the pixels in front of the first and behind the last image may be NaN or Inf patterns and come back bit for bit
 * (a kernel whose address range is wider than the view masks those lanes; it never multiplies them by a zero weight).  The same holds
 * for every entry point below that takes a pitch.  Documented exceptions: dy_conv2d_wgrad_nhwc and dy_colsum READ the tail of the
 * last 16-byte chunk of a pixel (see there); nothing writes outside its view.  tests/test_conv_containment_gpu.py and
 * tests/test_view_containment_gpu.py hold every dispatch leaf and every such entry point to it.
 */
typedef struct dy_conv_desc {
  const void* x;         /* input view base */
  const void* w;         /* packed weights [cout_pad][k_pad] */
  const float* bias;     /* [cout_pad] fp32 */
  const void* residual;  /* optional view (n,ho,wo,cout), pitch ld_res; NULL = none */
  void* y;               /* output view base */
  int32_t batch, h, w_in, cin, ld_x;
  int32_t ho, wo, cout, ld_y, ld_res;
  int32_t ksize, stride, pad;
  int32_t groups;        /* 1 = dense (MFMA path); >1 = grouped/depthwise direct kernel:
                            w is then [cout][ksize*ksize*(cin/groups)] unpadded */
  int32_t act;           /* dy_act */
  int32_t dtype;         /* dy_dtype of x, w, residual */
  int32_t out_f32;       /* 1: y is fp32 regardless of dtype (Detect logits) */
  int32_t k_pad, cout_pad;
  int32_t up2x;          /* 1: x is read through a fused 2x nearest upsample
                            (nn.Upsample(None,2,'nearest') folded into this conv's gather):
                            h,w_in are the UPSAMPLED dims, the buffer holds (h/2, w_in/2).
                            2: x is read ZERO-DILATED by 2 (logical (h, w_in) = 2x the buffer dims, value at even
                            (row, col) only, zero elsewhere): the gather of a stride-2 transposed convolution, used for
                            the input gradient of stride-2 layers.  DY_WLAYOUT_ROWS only, no x2. */
  /* Optional second source = Concat folded into the gather (conv.py:323-333): input
   * channels [0,cin_split) are read from x (through up2x if set), channels
   * [cin_split,cin) from x2 (never upsampled), pitch ld_x2.  x2 = NULL: single source. */
  const void* x2;
  int32_t ld_x2, cin_split;
  /* Weight layout.  DY_WLAYOUT_ROWS (0): the [cout_pad][k_pad] rows described above (any ksize/stride).
   * DY_WLAYOUT_HALO3X3 (1): dense 3x3, pad 1, stride 1 or 2, single source, cout % 4 == 0 — selects the
   * LDS-halo kernel.  Weights are then packed in MFMA-fragment order: with E = 16/elem_size,
   * KC = 4*E channels per chunk, BN = (cout > 32 ? 64 : 32), NF = BN/16, the element
   *   w[co = nt*BN + j*16 + lr][r][q][ci = c*KC + lq*E + e]
   * lives at ((((nt*ceil(cin/KC) + c)*9 + (r*3+q))*NF + j)*64 + lq*16 + lr)*E + e, zero where co >= cout
   * or ci >= cin.  k_pad / cout_pad are ignored; bias stays fp32[dy_conv_cout_pad(cout)].
   * DY_WLAYOUT_FRAG1X1 (2): dense 1x1, stride 1, no residual (x2 / up2x allowed) — selects the streaming
   * kernel.  Same fragment order with a single tap: BN = (cout > 64 ? 128 : cout > 16 ? 64 : 16), NF = BN/16,
   *   w[co = nt*BN + j*16 + lr][ci = c*KC + lq*E + e]  at  (((nt*ceil(cin/KC) + c)*NF + j)*64 + lq*16 + lr)*E + e.
   * Built for ceil(cin/KC) in {2,3,4,6,8,12}; cout <= 16 and fp32 output (out_f32 with a 16-bit dtype) only
   * for 2 chunks; anything else returns DY_ERR_UNSUPPORTED (pack such layers with DY_WLAYOUT_ROWS). */
  int32_t w_layout;
  /* DY_FP8 only (BASELINE config 5: fp8 weights / activations on the fp8 MFMA, fp32 accumulate).  Weights are quantised per OUTPUT
   * channel, activations with ONE scale for the whole network (e4m3 is a floating format: a per-tensor scale only has to keep
   * the values inside [2^-9, 448] * scale):
   *   y_real[co] = act( (sum q_x * q_w[co]) * w_scale[co] + bias[co] ) (+ q_res * act_scale);   y_q = sat_e4m3(y_real / act_scale)
   * w_scale: fp32[cout_pad], = act_scale * (weight scale of channel co); with out_f32 the result is y_real itself.
   * DY_WLAYOUT_ROWS only.  Ignored (may be NULL / 0) for the other dtypes. */
  const float* w_scale;
  float act_scale;
  /* Training forward in front of a train-mode BatchNorm (conv.py:49-51): optional pointer to that BatchNorm's dy_bn_desc.workspace.
   * A kernel built for it stores, from its epilogue, per-channel partial sums and sums of squares of the STORED output values there
   * (one slot per spatial workgroup, in the layout of dy_bn_train_fwd's own reduction pass, totals zeroed), so the batch statistics
   * need no pass of their own: dy_conv_stats_written() returns the number of slots the calling thread's last dy_conv2d_nhwc wrote
   * (0: the dispatched kernel has no such epilogue, nothing was touched) -- hand it to dy_bn_desc.partial_slabs.  NULL = off. */
  double* bn_stats;
  /* Storage type of y when it differs from `dtype` (mixed-precision plans of BASELINE config 5: an fp8 trunk in front of a 16-bit
   * Detect tail, a 16-bit layer handing over to the fp8 trunk).  0: y has type `dtype` (or fp32 with out_f32); k > 0: y has
   * dy_dtype k - 1.  Built in the flat-K kernel (csrc/conv_gemm_fk.hip, DY_WLAYOUT_ROWS) for DY_FP8 -> DY_F16 and DY_F16 -> DY_FP8
   * (act_scale > 0 then gives the output quantum: y_q = sat_e4m3(y_real / act_scale)); any other pair returns DY_ERR_UNSUPPORTED. */
  int32_t y_dtype1;
  /* Training backward (r05).  This convolution computes an INPUT gradient whose output IS the gradient dy that reaches the train-mode
   * BatchNorm + activation of the layer in front (conv.py:49-51 backwards; that layer's output has this convolution as its only consumer,
   * so nothing is added to dy afterwards).  With bnb_z != NULL a kernel built for it reads that layer's saved pre-BatchNorm map z beside
   * its own stores and leaves, in bn_stats (= that BatchNorm's dy_bn_desc.workspace), per-channel partial sums of
   *     du = dy * act'(u)  and  du * xhat,      xhat = (z - mean) * rstd,  u = gamma * xhat + beta,   dy as STORED,
   * in the slot layout of dy_bn_train_bwd's own reduction pass (totals zeroed): dy_conv_stats_written() > 0 then goes to
   * dy_bn_desc.partial_slabs of dy_bn_train_bwd, which skips its pass over dy and z.  0 slots: the dispatched kernel has no such epilogue
   * and touched nothing (built: the register-weight 3x3 kernel, 16-bit, stride 1, 64 or 128 channels in, cout % 64 == 0, no residual).
   * bnb_z: (n, ho, wo, cout) view of pitch bnb_ld_z and type `dtype`; bnb_act: dy_act of that layer; mean / rstd / gamma / beta: fp32[cout].
   * With bnb_z set, bn_stats is never used for the forward statistics. */
  const void* bnb_z;
  int32_t bnb_ld_z, bnb_act;
  const float* bnb_mean;
  const float* bnb_rstd;
  const float* bnb_gamma;
  const float* bnb_beta;
} dy_conv_desc;

/* Quantise a 16-bit / fp32 NHWC view to DY_FP8: dst_q = sat_e4m3(src / act_scale).  c % 16 == 0, views 16-byte aligned.
 * Replaces nothing in the reference (it has no fp8 path); it is the hand-over from the image stem (run in fp16) to the fp8 layers. */
int32_t dy_quantize_fp8_nhwc(const void* src, void* dst, int64_t rows, int32_t c, int32_t ld_src, int32_t ld_dst, int32_t src_dtype, float act_scale,
                             dy_stream_t stream);
/* Pack the fp32 master weights of a convolution into a dy_conv_desc weight layout, on the device, in ONE launch (training re-packs
 * every step; replaces the host-side pad / permute / flip / cast of hip_ops.PackedConv).  w: fp32, read through the element strides
 * (s_co, s_ci, s_r, s_q) of its (cout, cin, r, q) axes — any memory layout.  transpose_flip = 1 packs the weights of the convolution
 * that computes the INPUT gradient: W'[ci][co][r][q] = w[co][ci][k-1-r][k-1-q] (logical cout / cin swapped).  cin_logical > cin: the
 * packed convolution sees cin_logical input channels, the extra ones zero (the 3-channel image padded to one chunk).  dst: `dtype`
 * (not DY_FP8), exactly the element count of the layout (ROWS: dy_conv_cout_pad x dy_conv_k_pad; fragment layouts as documented
 * at dy_conv_desc.w_layout), padding written as zeros. */
int32_t dy_pack_conv_weights(const float* w, int64_t s_co, int64_t s_ci, int64_t s_r, int64_t s_q, int32_t cout, int32_t cin, int32_t ksize,
                             int32_t transpose_flip, int32_t cin_logical, void* dst, int64_t dst_elems, int32_t dtype, int32_t w_layout, dy_stream_t stream);
/* The same for MANY convolutions in ONE launch (a training step re-packs every layer's weights twice: forward and input-gradient
 * form, ~160 launches of ~5 us).  dy_pack_conv_weights_table validates the jobs (the arguments of dy_pack_conv_weights, one dtype)
 * and writes the launch table into HOST memory (dy_pack_conv_weights_table_bytes(n) bytes) plus the grid size; the caller copies it to
 * the device once; dy_pack_conv_weights_batched runs it (re-usable while the source / destination addresses stand; capturable). */
typedef struct dy_pack_job {
  const float* w;
  int64_t s_co, s_ci, s_r, s_q;
  int32_t cout, cin, ksize, transpose_flip, cin_logical, w_layout;
  void* dst;
  int64_t dst_elems;
} dy_pack_job;
int64_t dy_pack_conv_weights_table_bytes(int32_t n_jobs);
int32_t dy_pack_conv_weights_table(const dy_pack_job* jobs, int32_t n_jobs, int32_t dtype, void* table_host, int64_t table_bytes, int32_t* total_blocks);
int32_t dy_pack_conv_weights_batched(const void* table_dev, int32_t n_jobs, int32_t total_blocks, int32_t dtype, dy_stream_t stream);
int32_t dy_conv_k_pad(int32_t cin, int32_t ksize, int32_t dtype);
int32_t dy_conv_cout_pad(int32_t cout);
int32_t dy_conv2d_nhwc(const dy_conv_desc* d, dy_stream_t stream);
int32_t dy_conv_stats_written(void); /* > 0: slots of d->bn_stats the last dy_conv2d_nhwc of this thread filled */

/* Whether the kernels behind a special weight layout take a call is decided HERE and asked by the caller (hip_ops.py::PackedConv.for_call,
 * conv_pack_plan); the dispatch of dy_conv2d_nhwc runs the same functions.  Both are host arithmetic: they need no device, launch nothing
 * and never set the error string.
 *
 * dy_conv3x3_halo_route: which kernel a dense 3x3 pad-1 call on a DY_WLAYOUT_HALO3X3 pack runs.  x_bytes / y_bytes: extent of the input /
 * output view (batch * rows * cols * pitch * element size), ld_y in elements, y_addr: address of the output view, residual / out_f32:
 * 0 / 1 as in dy_conv_desc, gathered: 1 when the call has a second source (x2) or an upsampled / dilated gather (up2x != 0).
 * DY_ROUTE_ROWS: none of them takes it -- dy_conv2d_nhwc returns DY_ERR_UNSUPPORTED, run the call on the layer's DY_WLAYOUT_ROWS pack. */
typedef enum dy_conv_route { DY_ROUTE_ROWS = 0, DY_ROUTE_HREG = 1, DY_ROUTE_HREG_S2 = 2, DY_ROUTE_HALO = 3 } dy_conv_route;
int32_t dy_conv3x3_halo_route(int32_t cin, int32_t cout, int32_t stride, int32_t dtype, int64_t x_bytes, int64_t y_bytes, int32_t ld_y,
                              uint64_t y_addr, int32_t residual, int32_t out_f32, int32_t gathered);
/* dy_conv1x1_stream_supported: 1 when the streaming kernel behind DY_WLAYOUT_FRAG1X1 is built for a dense 1x1 stride-1 layer of this
 * shape (K groups, cout tile and LDS footprint of the build), out_f32: the layer will be called with dy_conv_desc.out_f32. */
int32_t dy_conv1x1_stream_supported(int32_t cin, int32_t cout, int32_t dtype, int32_t out_f32);

/* ---- one Detect branch from its second 3x3 convolution to the decoded output ------------------------------
 * Replaces in ONE kernel per (level, branch), 16-bit storage: Detect.forward's cv2[i][1] -> cv2[i][2] (kind 1, box) or cv3[i][1] ->
 * cv3[i][2] (kind 2, class) of the legacy v8 head (nn/modules/head.py:43-57, 64-70), each Conv = SiLU(conv + folded BatchNorm
 * bias) (conv.py:53-55), and that branch's share of Detect._inference (head.py:100-131): kind 1 = DFL (block.py:58-76) + dist2bbox on the
 * anchor grid (tal.py:333-357) x stride -> rows 0..3 of pred; kind 2 = sigmoid -> rows 4.. of pred + the NMS candidate filter
 * (ops.py:250,290-295: best class score > conf_thres, optional class mask) appended to the dy_nms workspace.
 * x: NHWC (batch, h, w, c_in) pitch ld_x, the output of the branch's FIRST conv.  w3 / b3: the 3x3 c_in -> c_mid conv in
 * DY_WLAYOUT_HALO3X3, bias fp32[64].  w1 / b1: the plain 1x1 conv in DY_WLAYOUT_FRAG1X1 (kind 1: c_mid -> 4*reg_max, bias fp32[64];
 * kind 2: c_mid -> nc <= 16, bias fp32[16] zero padded).  out: pred (batch, 4 + nc, anchors) fp32; this level's anchors are
 * [anchor0, anchor0 + h*w) in row-major (y, x) order.  kind 2 with nms_workspace: candidates are APPENDED — zero the counts once per
 * pass with dy_nms_reset_counts before the first class branch; then dy_nms(prefiltered = 1).
 * Built for c_in = c_mid = 64, reg_max 16, DY_BF16 / DY_F16 (dy_detect_branch_fused_supported tells). */
typedef struct dy_branch_desc {
  const void* x;
  const void* w3;
  const float* b3;
  const void* w1;
  const float* b1;
  float* out;
  int32_t batch, h, w, ld_x, c_in, c_mid, nc, reg_max, kind, dtype, anchors, anchor0;
  float stride;
  void* nms_workspace;
  int64_t nms_workspace_bytes;
  float conf_thres;
  const uint8_t* classes_mask;
  int32_t act_l2e; /* 1: the trunk conv's SiLU is DY_ACT_SILU_L2E (b3 scaled by log2 e, w1 divided by it: the logits stay in true units) */
} dy_branch_desc;
int32_t dy_detect_branch_fused_supported(int32_t c_in, int32_t c_mid, int32_t c_out, int32_t kind, int32_t nc, int32_t reg_max, int32_t dtype);
int32_t dy_detect_branch_fused(const dy_branch_desc* d, dy_stream_t stream);
int32_t dy_nms_reset_counts(void* nms_workspace, int32_t batch, dy_stream_t stream);

/* ---- fused C2f block (n = 1, hidden 32) -------------------------------------------------------------
 * Replaces in ONE kernel: C2f.forward (nn/modules/block.py:237-242) = cv1 (Conv 1x1 cin -> 2*hidden) -> chunk(2) ->
 * Bottleneck(hidden, hidden, shortcut, k = (3,3), e = 1.0) (block.py:337-350) -> cat -> cv2 (Conv 1x1 3*hidden -> cout), each
 * Conv = SiLU(conv + folded BatchNorm bias) (conv.py:53-55), for the stride-4 C2f blocks of Drone-YOLO-s: the backbone's
 * (yolov8-p2-repvgg.yaml layer 2) and, with cin_lo > 0, the neck's (layer 21) together with the nn.Upsample(2, 'nearest') and
 * Concat (conv.py:323-335) in front of it: the block input is then [upsample2x(x_lo) (cin_lo channels) | x (cin - cin_lo)].
 * Intermediates stay on chip, rounded to `dtype` where the layer-by-layer path rounds.
 * x: NHWC (batch, h, w, cin - cin_lo) pitch ld_x; x_lo: NHWC (batch, h/2, w/2, cin_lo) pitch ld_x_lo, or NULL with cin_lo = 0;
 * y: NHWC (batch, h, w, cout) pitch ld_y.  Weights (BatchNorm folded):
 *   w_cv1   DY_WLAYOUT_FRAG1X1 of (2*hidden, cin);      w_cv2   DY_WLAYOUT_FRAG1X1 of (cout, 3*hidden);
 *   w_m_cv1, w_m_cv2   DY_WLAYOUT_HALO3X3 of (hidden, hidden, 3, 3);
 *   bias    fp32: cv1 [2*hidden] | m.cv1 [hidden] | m.cv2 [hidden] | cv2 [cout].
 * Built for 64 direct channels (+ 128 upsampled), hidden 32, cout 64, DY_BF16 / DY_F16 (dy_c2f_fused_supported tells); other
 * shapes: run the four dy_conv2d_nhwc calls. */
typedef struct dy_c2f_desc {
  const void* x;
  const void* x_lo;
  void* y;
  const void* w_cv1;
  const void* w_m_cv1;
  const void* w_m_cv2;
  const void* w_cv2;
  const float* bias;
  int32_t batch, h, w, cin, cin_lo, hidden, cout, ld_x, ld_x_lo, ld_y, shortcut, dtype;
  int32_t act_l2e; /* 1: all four SiLUs are DY_ACT_SILU_L2E (input, output and biases in the log2(e)-scaled domain) */
} dy_c2f_desc;
int32_t dy_c2f_fused_supported(int32_t cin, int32_t cin_lo, int32_t hidden, int32_t cout, int32_t n_bottlenecks, int32_t dtype);
int32_t dy_c2f_fused(const dy_c2f_desc* d, dy_stream_t stream);

/* ---- tail of a hidden-64 C2f block: last Bottleneck 3x3 + closing 1x1 in ONE kernel ------------------------
 * Replaces, 16-bit storage: the last Bottleneck's cv2 (Conv 3x3 hidden -> hidden, block.py:337-350, with the shortcut add
 * x + cv2(cv1(x)) when `shortcut`) and C2f.forward's closing cv2 (Conv 1x1 (2 + n) * hidden -> cout over cat(y), block.py:237-242),
 * each Conv = SiLU(conv + folded BatchNorm bias) (conv.py:53-55), for the stride-8 blocks of Drone-YOLO-s (yaml layers 4, 15, 21).
 * t: NHWC (batch, h, w, hidden) pitch ld_t, the output of the last Bottleneck's cv1.  buf: the head of the concat buffer,
 * NHWC (batch, h, w, (1 + n) * hidden) pitch ld_buf = y0 | y1 | .. | y_n (y_n is the shortcut's source); the block's last
 * hidden channels (the fused 3x3's output) never reach memory.  y: NHWC (batch, h, w, cout) pitch ld_y (may be a channel slice).
 * w3 / b3: DY_WLAYOUT_HALO3X3 of (hidden, hidden, 3, 3), fp32[hidden].  w1 / b1: DY_WLAYOUT_FRAG1X1 of (cout, (2 + n) * hidden) in
 * C2f.cv2's input order (buffer channels first, the 3x3's output last), fp32[cout].  Intermediates are rounded to `dtype` where the
 * layer-by-layer path rounds them and summed in its order: the result is that of the two dy_conv2d_nhwc calls, bit for bit.
 * Built for hidden 64, cout 128, n 1 or 2, 3x3 / 3x3 Bottlenecks with groups 1, DY_BF16 / DY_F16 (dy_c2f_tail_fused_supported tells). */
typedef struct dy_c2f_tail_desc {
  const void* t;
  const void* buf;
  void* y;
  const void* w3;
  const float* b3;
  const void* w1;
  const float* b1;
  int32_t batch, h, w, hidden, cout, n_bottlenecks, shortcut, ld_t, ld_buf, ld_y, dtype;
  int32_t act_l2e; /* 1: both SiLUs are DY_ACT_SILU_L2E (inputs, output and biases in the log2(e)-scaled domain) */
} dy_c2f_tail_desc;
int32_t dy_c2f_tail_fused_supported(int32_t hidden, int32_t cout, int32_t n_bottlenecks, int32_t ksize1, int32_t ksize2, int32_t groups, int32_t dtype);
int32_t dy_c2f_tail_fused(const dy_c2f_tail_desc* d, dy_stream_t stream);

/* ---- front of a hidden-64 C2f block: the stride-2 3x3 in front of it + the block's opening 1x1 in ONE kernel ----
 * Replaces, 16-bit storage: a Conv / folded RepVGGBlock 3x3 stride 2 pad 1, cin -> cmid, whose only consumer is C2f.cv1 (Conv 1x1 ->
 * cout = 2 * hidden, block.py:237-242), directly (c_other = 0: yaml layers 3 -> 4 of Drone-YOLO-s) or as the FIRST source of a two-source
 * Concat (c_other channels from `other`: layers 19 -> 20 -> 21); each Conv = SiLU(conv + folded BatchNorm bias) (conv.py:53-55).
 * x: NHWC (batch, h, w, cin) pitch ld_x.  other: NHWC (batch, ho, wo, c_other) pitch ld_other, ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1
 * (NULL when c_other = 0).  y: NHWC (batch, ho, wo, cout) pitch ld_y (may be a channel slice).  The 3x3's output never reaches memory.
 * w3 / b3: DY_WLAYOUT_HALO3X3 of (cmid, cin, 3, 3), fp32[cmid].  w1 / b1: DY_WLAYOUT_FRAG1X1 of (cout, cmid + c_other) in cv1's input
 * order (the 3x3's output first), fp32[cout].  act: the activation code both convolutions would receive layer by layer, DY_ACT_SILU or
 * DY_ACT_SILU_L2E (inputs, output and biases in the log2(e)-scaled domain).  The intermediate is rounded to `dtype` where the layer-by-layer
 * path rounds it and both convolutions sum in that path's order: the result is that of the two dy_conv2d_nhwc calls, bit for bit.
 * Built for cin 64, (cmid, c_other) = (128, 0) or (64, 128), cout 128, DY_BF16 / DY_F16 (dy_c2f_front_fused_supported tells). */
typedef struct dy_c2f_front_desc {
  const void* x;
  const void* other;
  void* y;
  const void* w3;
  const float* b3;
  const void* w1;
  const float* b1;
  int32_t batch, h, w, cin, cmid, c_other, cout, ld_x, ld_other, ld_y, act, dtype;
} dy_c2f_front_desc;
int32_t dy_c2f_front_fused_supported(int32_t cin, int32_t cmid, int32_t c_other, int32_t cout, int32_t ksize, int32_t stride, int32_t groups, int32_t act, int32_t dtype);
int32_t dy_c2f_front_fused(const dy_c2f_front_desc* d, dy_stream_t stream);

/* Fused stem.  Replaces in one pass: the predictor's dtype/layout step for tensor sources
 * (engine/predictor.py:118-136) AND the model's first layer Conv(cin<=3, cout, 3, 2) (nn/modules/conv.py:37-55,
 * yolov8-p2-repvgg.yaml layer 0), so the image is never materialised in NHWC.
 * x: fp32 NCHW (n, cin, h, w) contiguous.  w: [ceil(cout/16)*16][32] of `dtype`, row co = the folded taps in
 * k = c*9 + r*3 + q order (i.e. OIHW flattened), zero padded to 32; bias fp32[ceil(cout/16)*16].
 * y: NHWC view (n, (h-1)/2+1, (w-1)/2+1, cout) of `dtype`, pitch ld_y.  cout <= 80.
 * DY_F16X2 (round 5): w = [cout_pad16][32] float16 hi halves, then as many lo halves, then fp32[cout_pad16] inverse row scales in ONE buffer
 * (rows scaled by a power of two into [2^13, 2^14) before the split, as for dy_conv2d_nhwc); the image is split on the fly; cout % 8 == 0, <= 64. */
int32_t dy_stem_conv3x3s2_nchw(const float* x, const void* w, const float* bias, void* y, int32_t n, int32_t cin,
                               int32_t h, int32_t w_in, int32_t cout, int32_t ld_y, int32_t act, int32_t dtype,
                               dy_stream_t stream);

/* The same from a uint8 NCHW image, value = x / divisor: the training input (DetectionTrainer.preprocess_batch's `img.float() / 255`,
 * models/yolo/detect/train.py:57-60) consumed by the stem directly.  16-bit storage, cout a multiple of 16 (<= 80); the operand values
 * are exactly those of dy_nchw_u8_to_nhwc followed by dy_conv2d_nhwc (same division, same rounding to `dtype`). */
int32_t dy_stem_conv3x3s2_nchw_u8(const uint8_t* x, float divisor, const void* w, const float* bias, void* y, int32_t n, int32_t cin,
                                  int32_t h, int32_t w_in, int32_t cout, int32_t ld_y, int32_t act, int32_t dtype, dy_stream_t stream);

/* Fused first TWO layers.  Replaces in one kernel: the layout step + Conv(3, 32, 3, 2) (yolov8-p2-repvgg.yaml layer 0,
 * nn/modules/conv.py:37-55) + RepVGGBlock(32, 64, stride 2) in deploy form (layer 1, nn/modules/block.py:1393-1490:
 * get_equivalent_kernel_bias folds the three branches into one 3x3 kernel), each followed by SiLU.  The 1/2-resolution
 * 32-channel intermediate stays in LDS, rounded to `dtype` exactly where the layer-by-layer path rounds it.
 * x: fp32 NCHW (n, 3, h, w) contiguous.  w0/b0: as dy_stem_conv3x3s2_nchw ([32][32], k = c*9 + r*3 + q; fp32[32]).
 * w1: [64][288] of `dtype`, k = (r*3 + q)*32 + c (BatchNorm and branches folded); b1: fp32[64].
 * y: NHWC view (n, h/4, w/4, 64) of `dtype`, pitch ld_y.  Built for DY_BF16 / DY_F16 and h, w multiples of 4
 * (dy_stem2_fused_supported tells); otherwise run dy_stem_conv3x3s2_nchw and dy_conv2d_nhwc.
 * DY_F16X2 (round 5): w0 = the split stem pack of dy_stem_conv3x3s2_nchw ([32][32] float16 hi halves, as many lo halves, fp32[32] inverse row
 * scales, one buffer); w1 = the split DY_WLAYOUT_ROWS pack of dy_conv2d_nhwc for a 3x3 32 -> 64 layer ([64][9 taps x 4 groups x (hi x 8 | lo x 8)]
 * float16) with its inverse row scales in w1_scale (fp32[64]); act0 = act1 = DY_ACT_SILU; y: split-float16 view, ld_y in 4-byte elements and
 * a multiple of 8.  The intermediate is rounded to (hi, lo) pairs where the layer-by-layer path rounds it. */
typedef struct dy_stem2_desc {
  const float* x;
  const void* w0;
  const float* b0;
  const void* w1;
  const float* b1;
  void* y;
  int32_t n, h, w, ld_y, act0, act1, dtype;
  const float* w1_scale; /* DY_F16X2 only (NULL otherwise) */
} dy_stem2_desc;
int32_t dy_stem2_fused_supported(int32_t cin, int32_t c0, int32_t c1, int32_t h, int32_t w, int32_t dtype);
int32_t dy_stem2_fused(const dy_stem2_desc* d, dy_stream_t stream);

/* ---- image sources: LetterBox + BGR->RGB + HWC->CHW + /255 ------------------------------------------
 * Replaces: LetterBox.__call__ (ultralytics/data/augment.py:1545-1608: cv2.resize INTER_LINEAR to (new_w, new_h), then
 * cv2.copyMakeBorder with 114) and the non-tensor branch of BasePredictor.preprocess (engine/predictor.py:125-135:
 * `im[..., ::-1].transpose(0,3,1,2)`, `.float()`, `/= 255`), in one pass.
 * src: DEVICE uint8 (n, h0, w0, 3), all frames one shape, channel order as decoded (BGR): swap_rb = 1 reverses it.
 * dst: fp32 (n, 3, hn, wn) contiguous = what dy_stem_conv3x3s2_nchw consumes.  The resized image occupies rows
 * [top, top+new_h) x columns [left, left+new_w); everything else is pad_value (114).  The geometry (new_w, new_h, top,
 * left, hn, wn) is LetterBox's own host arithmetic (augment.py:1566-1591).  8-bit bilinear arithmetic: OpenCV's
 * (11-bit coefficients), bit-exact against oracle/letterbox_oracle.py; new size == source size copies. */
int32_t dy_letterbox_u8_to_nchw_f32(const uint8_t* src, float* dst, int32_t n, int32_t h0, int32_t w0, int32_t new_w, int32_t new_h,
                                    int32_t top, int32_t left, int32_t hn, int32_t wn, int32_t swap_rb, float pad_value,
                                    dy_stream_t stream);

/* multi_scale of DetectionTrainer.preprocess_batch (models/yolo/detect/train.py:60-73): a uint8 NCHW batch -> fp32 NCHW (n, c, ho, wo) holding
 * nn.functional.interpolate(src.float() / 255, size=(ho, wo), mode="bilinear", align_corners=False) — torch's coordinate rule and blend order. */
int32_t dy_resize_bilinear_u8_nchw_f32(const uint8_t* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t ho, int32_t wo, dy_stream_t stream);
/* scale_img of test-time augmentation (utils/torch_utils.py:436-445, called by DetectionModel._predict_augment, nn/tasks.py:347-383): the fp32 NCHW batch
 * (n, c, h, w) — read mirrored left-right when flip_lr — resized bilinearly (align_corners = False, torch's coordinate rule) to (hs, ws) in the top-left
 * corner of dst (n, c, ho, wo), the rest filled with `pad` (the reference pads with 0.447 to multiples of the model's largest stride). */
int32_t dy_scale_img_nchw_f32(const float* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t hs, int32_t ws, int32_t ho, int32_t wo,
                              int32_t flip_lr, float pad, dy_stream_t stream);

/* ---- tiled inference on large frames -----------------------------------------------------------------
 * The reference slices through third-party packages that are not vendored (mix6.py:84-89 `sv.InferenceSlicer`,
 * examples/YOLOv8-SAHI-Inference-Video/yolov8_sahi.py:50-55): fixed-size tiles with a fractional overlap, one inference
 * per tile, detections shifted back and merged by class-aware NMS.  Parity is unpinned there; this build defines it.
 * dy_tiles_u8_to_nchw_f32: k crops (th x tw at offsets_yx[k] = (y, x), DEVICE int32) of ONE uint8 HWC frame (hf, wf, 3) ->
 *   fp32 (k, 3, th, tw) / 255 (swap_rb as in dy_letterbox_u8_to_nchw_f32); beyond the frame edge: pad_value.
 * dy_rows_to_pred: per-tile dy_nms outputs rows (k, max_det, 6) + counts (k) -> pred (1, 4+nc, k*max_det) fp32 in FRAME
 *   coordinates (xywh, the row's score in its class channel, zeros elsewhere and for rows >= counts) for a final dy_nms. */
int32_t dy_tiles_u8_to_nchw_f32(const uint8_t* frame, const int32_t* offsets_yx, float* dst, int32_t k, int32_t hf, int32_t wf, int32_t th,
                                int32_t tw, int32_t swap_rb, float pad_value, dy_stream_t stream);
int32_t dy_rows_to_pred(const float* rows, const int32_t* counts, const int32_t* offsets_yx, float* pred, int32_t k, int32_t max_det,
                        int32_t nc, dy_stream_t stream);

/* ---- tiled inference on batches of frames: batched slicer, one-launch merge (csrc/tile_merge.hip) -----------------
 * dy_tiles_batch_u8_to_nchw_f32: the slicer for f frames of one shape.  frames: uint8 (f, hf, wf, 3) contiguous; offsets_yx: k offsets
 *   (y, x), DEVICE int32, shared by all frames; dst: fp32 (f*k, 3, th, tw) / 255, frame-major (tile f*k + k'); swap_rb and pad_value as in
 *   dy_tiles_u8_to_nchw_f32, whose output it reproduces bit for bit (f = 1).  A lane handles four consecutive x of a tile row: float4
 *   stores when tw % 4 == 0 and dst is 16-byte aligned, scalar stores otherwise.
 * dy_tile_merge: the cross-tile merge of f frames in one launch, one workgroup per frame.
 *   rows: fp32 (f*k, max_det, 6) and counts: int32 (f*k): the per-tile dy_nms outputs, in tile pixels, clipped to the tile; offsets_yx (k, 2)
 *   as above.  Candidates are the rows r < counts[tile]; a candidate's box is the row's xyxy plus its tile's (ox, oy) (one fp32 add of an
 *   integer-valued float).  Order: descending score, ties by ascending slot k'*max_det + r.  Greedy suppression: a candidate is dropped when
 *   an already kept box of the same class (any class with agnostic; classes are compared as integers, nothing is added to coordinates) has
 *     metric 0 (IoU): inter / (area_i + area_j - inter) > thr      metric 1 (IoS): inter / fminf(area_i, area_j) > thr
 *   in fp32 without contraction, the IoU in dy_nms's expression order.  The scan stops at merge_max_det kept boxes.
 *   out: fp32 (f, merge_max_det, 6) = x1, y1, x2, y2 (clamped to [0, frame_w] x [0, frame_h]), conf, cls; rows >= count are zero.
 *   out_count: int32 (f).  out_index: optional int32 (f, merge_max_det): the slot of every kept row, -1 beyond the count; or NULL.
 *   nc: the number of classes of the rows (cls in [0, nc)).  workspace: dy_tile_merge_workspace_bytes(f, k, max_det) bytes, 16-byte aligned
 *   (-1 for sizes the entry point refuses).  Limits: k * max_det <= 32768 and merge_max_det <= 4096, DY_ERR_UNSUPPORTED beyond; every
 *   argument is checked before any launch.  The layout of out / out_count / out_index is dy_nms's, so dy_val_match and dy_track_step read it. */
int32_t dy_tiles_batch_u8_to_nchw_f32(const uint8_t* frames, const int32_t* offsets_yx, float* dst, int32_t f, int32_t k, int32_t hf, int32_t wf,
                                      int32_t th, int32_t tw, int32_t swap_rb, float pad_value, dy_stream_t stream);
typedef struct dy_tile_merge_desc {
  const float* rows;
  const int32_t* counts;
  const int32_t* offsets_yx;
  int32_t frames, tiles, max_det, nc;
  int32_t frame_h, frame_w;
  float thr;
  int32_t metric; /* 0 = IoU, 1 = IoS (intersection over the smaller area) */
  int32_t agnostic, merge_max_det;
  float* out;
  int32_t* out_count;
  int32_t* out_index;
  void* workspace;
  int64_t workspace_bytes;
} dy_tile_merge_desc;
int64_t dy_tile_merge_workspace_bytes(int32_t frames, int32_t tiles, int32_t max_det);
int32_t dy_tile_merge(const dy_tile_merge_desc* d, dy_stream_t stream);

/* dy_tile_fuse: dy_tile_merge whose kept rows absorb what they suppress (greedy non-maximum merging) instead of dropping it; one launch,
 *   one workgroup per frame, no host synchronisation.  Candidates, their frame-coordinate boxes, the order, the predicate and the kept rows
 *   are dy_tile_merge's: out_count, out_index, conf and cls of every output row are bit-identical to dy_tile_merge on the same input, only
 *   x1, y1, x2, y2 differ.  A candidate j that is not kept is absorbed by the kept row k of smallest index that stands before j in the
 *   sorted order and whose OWN box (never the grown one: greedy, not transitive) suppresses j; a candidate without such a row is dropped
 *   (only rows behind the stop at merge_max_det).  The members of a kept row are itself and the rows it absorbed.
 *     mode 1 (union): x1, y1 = the minimum, x2, y2 = the maximum over the members (exact in fp32, independent of order).
 *     mode 2 (wbf): a row with one member keeps its own box; otherwise, in integers (associative, bit-reproducible),
 *       w_j = (int64) rintf(score_j * 65536.f), q_jc = (int64) rintf(coord_jc * 64.f), S = sum w_j, X_c = sum w_j * q_jc,
 *       fused_c = (float)(((double)X_c / (double)S) * 0.015625); S == 0 keeps the row's own box.  frame_h, frame_w <= 32768
 *       (DY_ERR_UNSUPPORTED beyond: X_c stays below 2^53).
 *   Both are clamped to the frame like dy_tile_merge's rows.  out_members: int32 (f, merge_max_det), the number of members of every kept
 *   row (>= 1), 0 beyond the count.  No floating-point atomic anywhere: two launches on one input give bit-identical buffers.
 *   workspace: dy_tile_fuse_workspace_bytes(f, k, max_det, merge_max_det) bytes (the keys and 40 bytes of accumulators per output row;
 *   -1 for sizes the entry point refuses), 16-byte aligned.  Limits and checks as dy_tile_merge, and mode; all before any launch. */
typedef struct dy_tile_fuse_desc {
  const float* rows;
  const int32_t* counts;
  const int32_t* offsets_yx;
  int32_t frames, tiles, max_det, nc;
  int32_t frame_h, frame_w;
  float thr;
  int32_t metric; /* 0 = IoU, 1 = IoS */
  int32_t agnostic, merge_max_det;
  int32_t mode; /* 1 = union, 2 = wbf */
  float* out;
  int32_t* out_count;
  int32_t* out_index;   /* optional, as in dy_tile_merge_desc */
  int32_t* out_members;
  void* workspace;
  int64_t workspace_bytes;
} dy_tile_fuse_desc;
int64_t dy_tile_fuse_workspace_bytes(int32_t frames, int32_t tiles, int32_t max_det, int32_t merge_max_det);
int32_t dy_tile_fuse(const dy_tile_fuse_desc* d, dy_stream_t stream);

/* dy_tile_merge_rotated: the cross-tile merge of f frames for oriented boxes; one launch, one workgroup per frame, no host synchronisation.
 *   rows: fp32 (f*k, max_det, 7) = x, y, w, h, theta, conf, cls and counts: int32 (f*k): the per-tile dy_nms_rotated + dy_scale_rboxes
 *   outputs, in tile pixels; offsets_yx (k, 2) DEVICE int32 as for dy_tile_merge.  Candidates are the rows r < min(counts[tile], max_det)
 *   (a negative count is 0), slot = k'*max_det + r.  Order: descending conf, ties by ascending slot (key = ~bits(conf) << 32 | slot).
 *   A candidate's box is (x + ox, y + oy, w, h, theta): one fp32 add of an integer-valued float each; its covariance row (x, y, a, b, c of
 *   csrc/probiou.h's rnms_row) is computed once per candidate, never per pair.  A kept row i suppresses candidate j when
 *     (agnostic || cls_i == cls_j) && rnms_probiou(row_i, row_j) >= thr        (the kept row first; a NaN does not suppress)
 *   with the one ProbIoU expression of dy_nms_rotated and dy_val_match_rotated, fp32 without contraction.  Classes are compared as integers
 *   and NOTHING is added to the coordinates (dy_nms_rotated's max_wh class offset would cost ProbIoU its low bits at frame coordinates of
 *   several thousand pixels).  GREEDY, not fast: a candidate is tested only against rows that were kept, so a row that only a dropped
 *   duplicate overlaps survives -- dy_tile_merge's rule; dy_nms_rotated reproduces the reference's fast NMS, in which a suppressed row still
 *   suppresses, and the reference has no slicer to follow here.  The scan stops at merge_max_det kept rows.
 *   out: fp32 (f, merge_max_det, 7) in the input column order; x and w clamped to [0, frame_w], y and h to [0, frame_h] (clip_boxes on xywh
 *   rows, as dy_scale_rboxes); theta, conf, cls copied; rows >= count are zero.  out_count: int32 (f).  out_index: optional int32
 *   (f, merge_max_det): the slot of every kept row, -1 beyond the count; or NULL.  workspace: dy_tile_merge_rotated_workspace_bytes(f, k,
 *   max_det) bytes, 16-byte aligned (-1 for sizes the entry point refuses).  Limits: k * max_det <= 32768 and merge_max_det <= 4096
 *   (DY_ERR_UNSUPPORTED beyond), thr in [0, 1], DY_ERR_WORKSPACE for a short workspace; every argument is checked before any launch. */
typedef struct dy_tile_merge_rotated_desc {
  const float* rows;
  const int32_t* counts;
  const int32_t* offsets_yx;
  int32_t frames, tiles, max_det, nc;
  int32_t frame_h, frame_w;
  float thr; /* ProbIoU */
  int32_t agnostic, merge_max_det;
  float* out;
  int32_t* out_count;
  int32_t* out_index;
  void* workspace;
  int64_t workspace_bytes;
} dy_tile_merge_rotated_desc;
int64_t dy_tile_merge_rotated_workspace_bytes(int32_t frames, int32_t tiles, int32_t max_det);
int32_t dy_tile_merge_rotated(const dy_tile_merge_rotated_desc* d, dy_stream_t stream);

/* ---- frame masks of tiled segmentation (csrc/tile_merge.hip, csrc/mask_ops.hip) --------------------------
 * dy_tile_mask_owner: which kept frame row every per-tile candidate belongs to; one launch, no host synchronisation.
 *   rows / counts / offsets_yx / frames / tiles / max_det / thr / metric / agnostic / merge_max_det: what dy_tile_merge (or dy_tile_fuse)
 *   was given; kept_index int32 (f, merge_max_det) and kept_count int32 (f): its out_index and out_count.
 *   owner: int32 (f, tiles * max_det).  Slot j = k' * max_det + r:  r >= counts[tile] -> -1;  the slot of kept row t -> t;  otherwise, with
 *   stitch == 0, -1, and with stitch != 0 the smallest t such that kept row t stands before j in the merge's order (key = ~bits(conf) << 32 |
 *   slot ascending) and the OWN box of t (row xyxy plus tile offset, before the clamp) suppresses j under dy_tile_merge's predicate (the one
 *   expression of tile_merge.hip, fp32 without contraction) -- dy_tile_fuse's absorb rule: the histogram of owner is its out_members --
 *   or -1 when there is none.  Limits and codes as dy_tile_merge; every argument is checked before the launch.
 * dy_tile_process_mask: one uint8 0 / 1 mask per emitted kept row, assembled from per-tile prototypes and coefficient rows.
 *   protos: fp32 NHWC (f * tiles, mh, mw, 32), pitch ld_p, 16-byte aligned, mh * 4 == tile_h and mw * 4 == tile_w; side: the dy_mask_gather
 *   output (f * tiles, max_det, 36), boxes in tile pixels; counts, offsets_yx as above; owner from dy_tile_mask_owner (or hand-made);
 *   dest: int32 (f, merge_max_det): the index in [0, total) of the output mask of kept row t, -1: not emitted.
 *   out: uint8 (total, oh, ow), oh = ceil(frame_h / stride), ow = ceil(frame_w / stride), 4-byte aligned; every byte is defined on return
 *   (the call zeroes it on the stream, then ORs with 32-bit integer atomics: bit-reproducible).  Pixel (Y, X) of mask dest[f, t] is the OR
 *   over the slots j of frame f with owner[f, j] == t of member j's value: with (oy, ox) its tile's offset, in fp32,
 *     ty = ((float)Y + 0.5f) * stride - oy, tx likewise; 0 unless 0 <= ty < tile_h and 0 <= tx < tile_w;
 *     sy = max(0.25f * ty - 0.5f, 0), y0 = min((int)sy, mh - 1), y1 = min(y0 + 1, mh - 1), ly1 = sy - y0 (x likewise);
 *     the blend of the four corners > 0, a corner = the 32-term dot product of the row's coefficients and the proto pixel, counted as 0
 *     outside the crop window of the row's box * 0.25f on the (mh, mw) grid (a NaN corner: empty) -- dy_process_mask's expressions: at
 *     stride 1 a single-member row is dy_process_mask's (tile_h, tile_w) mask of its tile row pasted at (oy, ox), bit for bit.
 *   A slot with owner -1, dest -1 or r >= counts is neither read nor written.  total == 0: DY_OK without a launch.  nm != 32, a stride
 *   other than 1 / 2 / 4, a proto grid that is not a quarter of the tile: DY_ERR_UNSUPPORTED; oh * ow >= 2^31: DY_ERR_INVALID_ARG. */
typedef struct dy_tile_mask_owner_desc {
  const float* rows;
  const int32_t* counts;
  const int32_t* offsets_yx;
  const int32_t* kept_index;
  const int32_t* kept_count;
  int32_t frames, tiles, max_det, merge_max_det;
  float thr;
  int32_t metric, agnostic, stitch;
  int32_t* owner;
} dy_tile_mask_owner_desc;
int32_t dy_tile_mask_owner(const dy_tile_mask_owner_desc* d, dy_stream_t stream);

typedef struct dy_tile_process_mask_desc {
  const float* protos;
  const float* side;
  const int32_t* counts;
  const int32_t* offsets_yx;
  const int32_t* owner;
  const int32_t* dest;
  int32_t frames, tiles, max_det, merge_max_det, nm, mh, mw, ld_p, tile_h, tile_w, frame_h, frame_w, stride, total;
  uint8_t* out;
} dy_tile_process_mask_desc;
int32_t dy_tile_process_mask(const dy_tile_process_mask_desc* d, dy_stream_t stream);

/* ---- layout / copy ops ------------------------------------------------------ */

/* Replaces: predictor preprocess `.half()/.float()` + the NCHW->device layout step
 * (engine/predictor.py:118-136).  src: fp32 NCHW (n,c,h,w) contiguous.  dst: NHWC
 * view of `dtype`, pitch ld_dst, channels [c, c_pad) are written as zero. */
int32_t dy_nchw_f32_to_nhwc(const float* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w,
                            int32_t c_pad, int32_t ld_dst, int32_t dtype, dy_stream_t stream);

/* Training input: uint8 NCHW batch -> NHWC of `dtype`, every value divided by `divisor` (255), channels zero-padded to c_pad.
 * Replaces DetectionTrainer.preprocess_batch's `batch["img"].float() / 255` (models/yolo/detect/train.py:57-60) + the
 * layout step, in one pass (1 byte read per value). */
int32_t dy_nchw_u8_to_nhwc(const uint8_t* src, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, int32_t c_pad,
                           int32_t ld_dst, float divisor, int32_t dtype, dy_stream_t stream);

/* Inverse, for handing activations back to NCHW callers: src NHWC view -> fp32 NCHW. */
int32_t dy_nhwc_to_nchw_f32(const void* src, float* dst, int32_t n, int32_t c, int32_t h, int32_t w,
                            int32_t ld_src, int32_t src_dtype, dy_stream_t stream);

/* Replaces: nn.Upsample(None, 2, 'nearest') feeding Concat (yolov8-p2-repvgg.yaml:30,34,38).
 * src (n,h,w,c) pitch ld_src -> dst (n,2h,2w,c) pitch ld_dst (typically a channel
 * slice of the Concat buffer). c % (16/elem_size) == 0. */
int32_t dy_upsample2x_nhwc(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c,
                           int32_t ld_src, int32_t ld_dst, int32_t dtype, dy_stream_t stream);

/* Strided NHWC copy (Concat fallback when a producer could not write in place;
 * conv.py:323-333). */
int32_t dy_copy_nhwc(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c,
                     int32_t ld_src, int32_t ld_dst, int32_t dtype, dy_stream_t stream);

/* Replaces: SPPF's three chained MaxPool2d(k,1,k//2) (nn/modules/block.py:185-191).
 * x: (n,h,w,c) pitch ld.  y1,y2,y3: pooled once/twice/thrice, same pitch ld (the
 * channel slices of the SPPF concat buffer).  k odd, (k/2)*3 halo; h*w*16B*3 must
 * fit LDS (h*w <= 4608; a workgroup takes up to eight 16-byte channel chunks of one image: whole lines). */
int32_t dy_sppf_maxpool3(const void* x, void* y1, void* y2, void* y3, int32_t n, int32_t h, int32_t w,
                         int32_t c, int32_t ld, int32_t k, int32_t dtype, dy_stream_t stream);

/* ---- Detect decode ------------------------------------------------------------
 * Replaces: Detect._inference (nn/modules/head.py:100-131) = DFL (block.py:58-76) +
 * make_anchors (utils/tal.py:333-345) + dist2bbox xywh (tal.py:348-357) * stride +
 * sigmoid(cls), concatenated to (batch, 4+nc, A).
 * Per level l the raw head output is an fp32 NHWC view (n, h_l, w_l, 4*reg_max + nc)
 * with pitch ld_l: channels [0,4*reg_max) are the box bins, the next nc the class logits.
 * out: fp32 (batch, 4+nc, A) contiguous, A = sum_l h_l*w_l, levels in order. */
#define DY_MAX_LEVELS 8
typedef struct dy_decode_desc {
  const float* level[DY_MAX_LEVELS];
  int32_t h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS];
  float stride[DY_MAX_LEVELS];
  int32_t n_levels, batch, nc, reg_max;
  float* out;
  /* Optional fusion of the NMS candidate filter (ops.py:250,290-295) into the decode pass: when
   * nms_workspace != NULL (a dy_nms workspace for the same batch/anchors) every anchor whose best class
   * score > conf_thres (and passes classes_mask) is appended to it, and dy_nms can then be called with
   * prefiltered = 1 on `out`, skipping its own pass over the predictions. */
  void* nms_workspace;
  int64_t nms_workspace_bytes;
  float conf_thres;
  const uint8_t* classes_mask;
} dy_decode_desc;
int32_t dy_detect_decode(const dy_decode_desc* d, dy_stream_t stream);

/* ---- fused Detect tail: last 1x1 convs of both branches + decode (+ NMS filter) ---------------
 * Replaces in ONE pass, per level l: cv2[l][2] = nn.Conv2d(c_box, 4*reg_max, 1) and cv3[l][2] =
 * nn.Conv2d(c_cls, nc, 1) (nn/modules/head.py:43-57), their concat (head.py:69-70) and Detect._inference
 * (head.py:100-131), i.e. dy_conv2d_nhwc x2 + dy_detect_decode without the (batch, 4*reg_max+nc, A) fp32
 * logits ever reaching HBM.  Inference only: the raw per-level maps the reference also returns (head.py:74)
 * are not produced (use the unfused calls when they are wanted, e.g. for the training loss).
 * x_box[l] / x_cls[l]: NHWC views (batch, h_l, w_l, c_box / c_cls) of `dtype`, pitches ld_box / ld_cls —
 * the outputs of cv2[l][1] / cv3[l][1].  w_box[l] / w_cls[l]: the 1x1 weights packed as DY_WLAYOUT_FRAG1X1
 * for (cout = 4*reg_max, cin = c_box) / (cout = nc, cin = c_cls); b_box / b_cls: fp32 bias padded like there.
 * out, nms_workspace, conf_thres, classes_mask: exactly as in dy_decode_desc.
 * Built for reg_max 16, nc <= 128, c_box = 64, c_cls in {64, 96, 128, 160} (16-bit) or {64, 80} (fp32);
 * dy_detect_head_decode_supported() tells (1/0); unsupported shapes return DY_ERR_UNSUPPORTED.
 * DY_F16X2 (round 5; c_box = 64, c_cls in {64, 96, 128}): x_box / x_cls are split-float16 views; w_box[l] / w_cls[l] hold the float16
 * DY_WLAYOUT_FRAG1X1 image (k-groups of 32 channels) of the hi halves followed by the image of the lo halves (rows scaled by a power of
 * two into [2^13, 2^14) first, as for dy_conv2d_nhwc); b_box[l] / b_cls[l] hold the padded bias followed by as many inverse row scales. */
typedef struct dy_head_decode_desc {
  const void* x_box[DY_MAX_LEVELS];
  const void* x_cls[DY_MAX_LEVELS];
  const void* w_box[DY_MAX_LEVELS];
  const void* w_cls[DY_MAX_LEVELS];
  const float* b_box[DY_MAX_LEVELS];
  const float* b_cls[DY_MAX_LEVELS];
  int32_t ld_box[DY_MAX_LEVELS], ld_cls[DY_MAX_LEVELS], h[DY_MAX_LEVELS], w[DY_MAX_LEVELS];
  float stride[DY_MAX_LEVELS];
  int32_t n_levels, batch, nc, reg_max, c_box, c_cls, dtype;
  float* out;
  void* nms_workspace;
  int64_t nms_workspace_bytes;
  float conf_thres;
  const uint8_t* classes_mask;
} dy_head_decode_desc;
int32_t dy_detect_head_decode_supported(int32_t c_box, int32_t c_cls, int32_t nc, int32_t reg_max, int32_t dtype);
int32_t dy_detect_head_decode(const dy_head_decode_desc* d, dy_stream_t stream);

/* ---- NMS --------------------------------------------------------------------
 * Replaces: ops.non_max_suppression (utils/ops.py:181-332; the predictor's single-label path and the validator's multi_label path)
 * including torchvision.ops.nms (called at ops.py:312): candidates = anchors
 * whose best class score > conf_thres; xywh -> xyxy; if more than max_nms keep the
 * max_nms best; boxes offset by cls*max_wh unless agnostic; greedy NMS in
 * descending score order (ties: lower anchor index first), suppress when
 * IoU > iou_thres; first max_det survivors are emitted.
 * pred: fp32 (batch, 4+nc(+nm), A) contiguous (the decode output).
 * classes_mask: optional host-independent DEVICE array of nc bytes (1 = keep class) or NULL.
 * out: fp32 (batch, max_det, 6): x1,y1,x2,y2,conf,cls; rows >= count are zero.
 * out_count: int32 (batch).  out_index: optional int32 (batch, max_det) anchor index of
 * every kept row (for parity tests / mask gathers) or NULL.
 * workspace: dy_nms_workspace_bytes(batch, A) bytes, 16-byte aligned.
 */
typedef struct dy_nms_desc {
  const float* pred;
  int32_t batch, nc, n_extra, anchors;
  float conf_thres, iou_thres;
  int32_t max_det, max_nms;
  float max_wh;
  int32_t agnostic;
  const uint8_t* classes_mask;
  float* out;
  int32_t* out_count;
  int32_t* out_index;
  void* workspace;
  int64_t workspace_bytes;
  int32_t prefiltered; /* 1: the workspace already holds the candidates (dy_detect_decode fused filter,
                          same conf_thres / classes_mask); only sort + suppress run */
  int32_t multi_label; /* 1 (and nc > 1): the validator's NMS (utils/ops.py:255, 286-288; call site models/yolo/detect/val.py:93-106):
                          every (anchor, class) pair scored above conf_thres is a candidate of its own (ties: ascending
                          anchor * nc + class, the reference's row-major torch.where order); out_index still names the ANCHOR.
                          The workspace is then dy_nms_workspace_bytes(batch, anchors * nc) bytes; not with prefiltered */
} dy_nms_desc;
int64_t dy_nms_workspace_bytes(int32_t batch, int32_t anchors);
int32_t dy_nms(const dy_nms_desc* d, dy_stream_t stream);
/* Images with at most this many candidates are sorted and scanned by the small suppress kernel (256 threads, about 22 KB of LDS at
 * max_det 300, so that another stream's convolution workgroups share the CU); images with more take the 1024-thread kernel.
 * Which kernel serves an image is decided on the device; the results are the same. */
int32_t dy_nms_small_cap(void);

/* Replaces: ops.scale_boxes + ops.clip_boxes (utils/ops.py:92-127, 335-354) as applied by
 * DetectionPredictor.construct_result (models/yolo/detect/predict.py:59-73) to the kept rows.
 * boxes: fp32 (batch, max_det, 6), updated in place for rows < counts[b]:
 *   x = clamp((x - pad_x) / gain, 0, clip_w),  y = clamp((y - pad_y) / gain, 0, clip_h).
 * params: DEVICE fp32 (batch, 5) = gain, pad_x, pad_y, clip_w, clip_h per image. */
int32_t dy_scale_boxes(float* boxes, const int32_t* counts, const float* params, int32_t batch,
                       int32_t max_det, dy_stream_t stream);

/* ---- oriented boxes (the reference's `obb` task, prediction) ------------------------------------------
 * All three are plain launches: no host synchronisation, no allocation, every argument checked before any launch, so they can be
 * recorded in a launch plan and captured in a hipGraph.  fp32 in the reference's order of operations, contraction off; expf / logf /
 * sinf / cosf are the device's.
 *
 * dy_obb_decode.  Replaces: OBB.forward's angle = (cv4(x).sigmoid() - 0.25) * pi (nn/modules/head.py:217-221) and OBB.decode_bboxes =
 * dist2rbox (utils/tal.py), behind the Detect kernels, whose decode already wrote cx = (ax + xf) s, cy = (ay + yf) s and wh into pred:
 *   theta[b, a] = (sigmoid(level[l][b, y, x, 0]) - 0.25) * pi
 *   (x, y)      = a s + R(theta) ((cx, cy) - a s),  a s = ((col + 0.5) s, (row + 0.5) s)      rows 0 and 1 of pred, in place
 * level[i]: fp32 NHWC (batch, h[i], w[i], >= 1 channels) with pixel pitch ld[i]: the raw angle logits in true units (channel 0 is read);
 * anchors are numbered level by level, row-major.  pred: fp32 (batch, 4 + nc + n_extra, anchors); rows 2.. are not touched.
 * theta: fp32 (batch, anchors). */
typedef struct dy_obb_decode_desc {
  const float* level[DY_MAX_LEVELS];
  int32_t h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS];
  float stride[DY_MAX_LEVELS];
  int32_t n_levels, batch, nc, n_extra, anchors;
  float* pred;
  float* theta;
} dy_obb_decode_desc;
int32_t dy_obb_decode(const dy_obb_decode_desc* d, dy_stream_t stream);

/* dy_nms_rotated.  Replaces: ops.non_max_suppression(..., rotated=True) on the predictor's single-label path (utils/ops.py:257-313) with
 * nms_rotated (:146-178) and batch_probiou (utils/metrics.py:178-275).  The descriptor is dy_nms's and so is the candidate stage: the
 * filter (or a `prefiltered` workspace of the fused Detect filter), the keys, the order (descending score, then ascending anchor) and the
 * max_nms truncation.  Boxes are (x + c, y + c, w, h, theta[b, anchor]) with c = cls * max_wh (0 with agnostic).  Suppression is the
 * reference's FAST NMS, not a greedy scan: in score order candidate j is kept iff NO candidate i < j of the image has
 * probiou(i, j) >= iou_thres, whether or not i was itself suppressed; the first max_det kept are emitted.
 * out: fp32 (batch, max_det, 7) = x, y, w, h, theta, conf, cls (the column order of OBBPredictor.construct_result); rows >= count are zero.
 * out_count (batch); out_index: optional (batch, max_det) anchors, -1 behind the count.
 * workspace: dy_nms_rotated_workspace_bytes(batch, anchors) bytes; its head IS a dy_nms workspace (what the fused filter fills), behind it
 * lies the table of the images with more than dy_nms_rotated_lds_cap() candidates.  multi_label: DY_ERR_UNSUPPORTED. */
int64_t dy_nms_rotated_workspace_bytes(int32_t batch, int32_t anchors);
int32_t dy_nms_rotated(const dy_nms_desc* d, const float* theta, dy_stream_t stream);
int32_t dy_nms_rotated_lds_cap(void);

/* dy_nms_rotated_ml.  Replaces: ops.non_max_suppression(..., rotated=True, multi_label=True), the validator's NMS of an oriented-box model
 * (models/yolo/detect/val.py postprocess with task == "obb"; utils/ops.py:286-288: `i, j = torch.where(cls > conf_thres)`).  An entry point
 * of its own beside dy_nms_rotated: every (anchor, class) pair scored above conf is a candidate, whatever d->multi_label says; nc == 1
 * degrades to the single-label form (ops.py:255).  The candidate stage is dy_nms's multi_label one: key low word anchor * nc + class, order
 * descending score, then ascending anchor * nc + class (the row-major order of the reference's torch.where).  Suppression, table (LDS up
 * to dy_nms_rotated_lds_cap() candidates, the workspace beyond that, decided on the device), the stop at max_det and the outputs are
 * dy_nms_rotated's; the class offset and column 6 of a row are the pair's class, out_index holds the pair's anchor.
 * workspace: dy_nms_rotated_ml_workspace_bytes(batch, anchors, nc) = a dy_nms workspace of anchors * nc candidates and a table of that
 * capacity.  prefiltered: DY_ERR_UNSUPPORTED (the fused Detect filter is single-label).  anchors * nc < 2^30. */
int64_t dy_nms_rotated_ml_workspace_bytes(int32_t batch, int32_t anchors, int32_t nc);
int32_t dy_nms_rotated_ml(const dy_nms_desc* d, const float* theta, dy_stream_t stream);

/* dy_scale_rboxes.  Replaces: OBBPredictor.construct_result (models/yolo/obb/predict.py:43-45) on the kept rows, in place for rows <
 * counts[b]: ops.regularize_rboxes (utils/ops.py:791-807: w and h swap iff theta mod pi >= pi / 2, then theta mod pi / 2, Python's `%`
 * for negative theta) and ops.scale_boxes(..., xywh=True) (:92-127): x = (x - pad_x) / gain, y = (y - pad_y) / gain, w / gain, h / gain,
 * then clip_boxes, which clamps columns 0 and 2 to [0, clip_w] and 1 and 3 to [0, clip_h] -- the WIDTH and HEIGHT too, as the reference does.
 * rows: fp32 (batch, max_det, 7) of dy_nms_rotated.  params: DEVICE fp32 (batch, 5) as for dy_scale_boxes. */
int32_t dy_scale_rboxes(float* rows, const int32_t* counts, const float* params, int32_t batch, int32_t max_det, dy_stream_t stream);

/* ---- validation matching on the padded NMS output ------------------------------------------------------
 * Replaces: BaseValidator.match_predictions (engine/validator.py:224-264, the non-scipy branch) and the box_iou it is fed
 * (utils/metrics.py:52-71), with the clip of the predictions to the image (_prepare_pred, models/yolo/detect/val.py:119-124), for a
 * whole batch in one launch behind dy_nms; no host synchronisation, capturable in a hipGraph.
 * rows: fp32 (batch, max_det, 6) and counts: int32 (batch): the dy_nms outputs (rows >= counts[i] are not read).
 * tbox: fp32 (n_labels, 4) label boxes, xyxy in pixels, already clipped, 16-byte aligned; tcls: fp32 (n_labels) their classes;
 * timg: int32 (n_labels) the image each label belongs to (by value: the labels need not be sorted).  n_labels = 0 with null label
 * pointers is valid.  iouv: HOST array of n_iouv (1..16) IoU thresholds, read during the call.
 * For detection d (clipped to [0, clip_w] x [0, clip_h]; class 0 with single_cls) and the labels l of its image:
 *   m(l, d) = box_iou(l, d) if tcls[l] == cls[d] else 0, in fp32 in box_iou's order of operations (bit-equal to the host's);
 *   best(d) = argmax_l m(l, d), biou(d) = max_l m(l, d); exact ties go to the label that comes first in tbox (the reference's order on
 *   exact ties comes from an unstable sort and is not defined);
 *   tp[d][i] = biou(d) >= iouv[i] and no d' < d of the image has best(d') == best(d) and biou(d') >= iouv[i].
 * tp: uint8 (batch, max_det, n_iouv).  best_iou: optional fp32 (batch, max_det) = biou; best_label: optional int32 (batch, max_det) =
 * position of best(d) in tbox, -1 when the image has no label.  Every element is written: rows >= counts[i] get 0 / 0 / -1.
 * max_det <= 4096 (32 bytes of LDS per detection).  One workgroup per image; labels per image are unbounded. */
typedef struct dy_val_match_desc {
  const float* rows;
  const int32_t* counts;
  const float* tbox;
  const float* tcls;
  const int32_t* timg;
  const float* iouv;
  int32_t batch, max_det, n_labels, n_iouv;
  float clip_w, clip_h;
  int32_t single_cls;
  uint8_t* tp;
  float* best_iou;
  int32_t* best_label;
} dy_val_match_desc;
int32_t dy_val_match(const dy_val_match_desc* d, dy_stream_t stream);

/* dy_val_match_rotated.  Replaces: OBBValidator._process_batch (models/yolo/obb/val.py: match_predictions on batch_probiou(gt, det)) with
 * the clip of its _prepare_pred, behind dy_nms_rotated / dy_nms_rotated_ml.  dy_val_match's descriptor, rule and outputs, except:
 * rows: fp32 (batch, max_det, 7) = x, y, w, h, theta, conf, cls.
 * tbox: fp32 (n_labels, 8), 16-byte aligned: x, y, w, h, theta in pixels / radians, already scaled and clipped, and three unused floats.
 * A detection is clipped as scale_boxes(xywh=True) at gain 1, pad 0 leaves it: x and w to [0, clip_w], y and h to [0, clip_h] (clip_boxes
 * clamps the width and height of an xywh row too); theta is untouched and not regularized.
 *   m(l, d) = probiou(label l, detection d) if tcls[l] == cls[d] (0 with single_cls) else 0, in fp32 in batch_probiou's order of operations
 *   (the expression of dy_nms_rotated; the device's sinf / cosf / logf / expf are not bit-equal to the host's); a NaN m never becomes the
 *   best, and a row without a best label gets 0 / 0 / -1.  36 bytes of LDS per detection. */
typedef dy_val_match_desc dy_val_match_rotated_desc;
int32_t dy_val_match_rotated(const dy_val_match_rotated_desc* d, dy_stream_t stream);

/* ---- training loss (forward + gradient w.r.t. the head outputs) -----------------------------------------------------
 * Replaces: v8DetectionLoss.__call__ (utils/loss.py:206-260) = TaskAlignedAssigner (utils/tal.py:14-295, topk /
 * alpha / beta as given) + BCE class loss + CIoU box loss (utils/metrics.py:74-134) + DFL (loss.py:65-113), on the
 * raw head outputs Detect returns in training mode (head.py:71-72).
 * level[l]: fp32 NHWC view (batch, h_l, w_l, 4*reg_max + nc), pitch ld_l (the Detect head buffers).
 * gt: DEVICE fp32 (batch, gmax, 5) = class, x1, y1, x2, y2 in input pixels, zero rows = padding (the output of
 * v8DetectionLoss.preprocess, loss.py:180-195).  out: fp32[4] = box, cls, dfl (after gains), total = sum * batch.
 * out_owner: optional int32 (batch, A): index of the ground-truth box each anchor is assigned to, or -1.
 * Assignment is sparse (no (batch, gmax, A) tensors).
 * grad_level[l] (optional, all or none): fp32 NHWC (batch, h_l, w_l, 4*reg_max + nc), pitch ld_grad[l]; receives
 * d total / d level[l] — what loss.backward() hands to the Detect head in the reference trainer (engine/trainer.py:381-389)
 * (alignment padding of a row — ld_grad[l] − (4*reg_max + nc) < 8 floats — may be overwritten with zeros: whole-line stores);
 * the assignment, soft targets, target_scores_sum and CIoU's alpha are constants exactly as under autograd
 * (tal.py:60 no_grad, metrics.py:127-128). */
typedef struct dy_loss_desc {
  const float* level[DY_MAX_LEVELS];
  int32_t h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS];
  float stride[DY_MAX_LEVELS];
  int32_t n_levels, batch, nc, reg_max;
  const float* gt;
  int32_t gmax, topk;
  float alpha, beta, box_gain, cls_gain, dfl_gain;
  float* out;
  int32_t* out_owner;
  void* workspace;
  int64_t workspace_bytes;
  float* grad_level[DY_MAX_LEVELS];
  int32_t ld_grad[DY_MAX_LEVELS];
} dy_loss_desc;
int64_t dy_detection_loss_workspace_bytes(int32_t batch, int32_t anchors, int32_t gmax, int32_t topk);
int32_t dy_detection_loss(const dy_loss_desc* d, dy_stream_t stream);

/* ---- oriented-box training loss (forward + gradient w.r.t. the head outputs and the angle logits) ---------------------
 * Replaces: v8OBBLoss.__call__ (utils/loss.py:638-708) = RotatedTaskAlignedAssigner (utils/tal.py:298-330 on :14-295: the anchor
 * centre inside the rotated rectangle, edges included; overlap = probiou(gt, pred).clamp(0) on pixel-unit xywhr) + BCE class loss +
 * RotatedBboxLoss (loss.py:116-137: 1 - probiou(pred, target / stride) in grid units, DFL against the UNROTATED box of the target's
 * xywh) on the (feats, angle) pair OBB returns in training mode (head.py:200-227), and its autograd.
 * level[l], grad_level[l], out, out_owner, workspace, the gains, topk / alpha / beta: as in dy_loss_desc.
 * angle[l]: fp32 NHWC view (batch, h_l, w_l, >= 1), pitch ld_angle[l]; channel 0 is the raw angle logit z, theta = (sigmoid(z) - 0.25) pi.
 * gt: DEVICE fp32 (batch, gmax, 6) = class, x, y, w, h in input pixels, r in radians; a row with x + y + w + h + r <= 0 is padding
 * (mask_gt, loss.py:664: a real label with such a sum is masked all the same).
 * grad_angle[l] (with grad_level, all or none): fp32 (batch, h_l, w_l) rows of pitch ld_grad_angle[l] <= 64 floats; every row is written
 * WHOLE on every call: d total / d z in channel 0 (0 for a background anchor), zeros behind it.  Nothing synchronises the host; the launch
 * sequence can be captured into a hipGraph. */
typedef struct dy_obb_loss_desc {
  const float* level[DY_MAX_LEVELS];
  const float* angle[DY_MAX_LEVELS];
  int32_t h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS], ld_angle[DY_MAX_LEVELS];
  float stride[DY_MAX_LEVELS];
  int32_t n_levels, batch, nc, reg_max;
  const float* gt;
  int32_t gmax, topk;
  float alpha, beta, box_gain, cls_gain, dfl_gain;
  float* out;
  int32_t* out_owner;
  void* workspace;
  int64_t workspace_bytes;
  float* grad_level[DY_MAX_LEVELS];
  float* grad_angle[DY_MAX_LEVELS];
  int32_t ld_grad[DY_MAX_LEVELS], ld_grad_angle[DY_MAX_LEVELS];
} dy_obb_loss_desc;
int64_t dy_obb_loss_workspace_bytes(int32_t batch, int32_t anchors, int32_t gmax, int32_t topk);
int32_t dy_obb_loss(const dy_obb_loss_desc* d, dy_stream_t stream);
/* The angle tail's dz from dy_obb_loss's grad_angle map: g fp32, channel 0 of `rows` rows of pitch ld_g; dz: rows of 8 channels of `dtype`
 * (DY_BF16 / DY_F16 / DY_F32; pitch ld_dz >= 8, whole 16-byte chunks) = g * (*scale, a DEVICE fp32 value, or 1 when scale is null) in
 * channel 0, zeros in channels 1..7: the one-channel 1x1 convolution of the OBB head padded to a width the convolution gradients serve. */
int32_t dy_obb_angle_grad_cast(const float* g, int32_t ld_g, int64_t rows, const float* scale, void* dz, int32_t ld_dz, int32_t dtype, dy_stream_t stream);

/* ---- segmentation training loss: the mask term (forward + gradient w.r.t. the mask coefficients and the prototypes) ------------
 * Replaces: the mask part of v8SegmentationLoss.__call__ (utils/loss.py:334-350), calculate_segmentation_loss and single_mask_loss
 * (loss.py:354-443) and crop_mask (utils/ops.py:660-676), overlap_mask = True, and their autograd.  The box, class and DFL terms and the
 * assignment stay with dy_detection_loss, called in front of it: `owner` is its out_owner, `gt` its label table.
 * owner: DEVICE int32 (batch, A): the label row of every anchor, < 0 = background.  The foreground set is owner >= 0, i.e. the anchors whose
 * alignment metric is positive (the reference's fg_mask may also hold picks at metric 0, whose choice follows torch.topk's tie order).
 * gt: DEVICE fp32 (batch, gmax, 5) = class, x1, y1, x2, y2 in input pixels.  img_h, img_w: the input size in pixels.
 * coef[l]: fp32 NHWC view (batch, h_l, w_l, nm) of pitch ld_coef[l] (a multiple of 4, 16-byte aligned): the outputs of Segment.cv4[l]; anchors
 * are numbered level by level, row-major, as in dy_loss_desc.  proto: NHWC (batch, mh, mw, nm) of proto_dtype (DY_BF16 / DY_F16 / DY_F32),
 * pitch ld_proto.  nm must be 32 (DY_ERR_UNSUPPORTED otherwise).
 * masks: (batch, gh, gw) overlap index maps, mask_dtype DY_MASK_U8 or DY_MASK_I32: value k + 1 = row k of that image in gt (padding rows in
 * the middle count as rows), 0 = nothing.  (mh, mw) = (gh, gw), or exactly twice it: then prototype pixel (y, x) reads map pixel (y >> 1, x >> 1),
 * F.interpolate(mode="nearest") at scale 2; any other ratio: DY_ERR_UNSUPPORTED.
 * Per foreground anchor a of image b with label row g: logit(p) = coef[a] . proto[b, p, :], target(p) = (masks[b, p] == g + 1), l(p) the BCE
 * with logits in its stable form; the crop is the LABEL's box on the prototype grid: column r is in iff r >= x1m && r < x2m with
 * x1m = (x1 / img_w) * mw in fp32 in that order, rows alike; term = sum_crop l / (mh * mw) / area, area = (x2/img_w - x1/img_w) *
 * (y2/img_h - y1/img_h); seg = box_gain * sum(term) / n_fg (0 with n_fg = 0, and every gradient 0).
 * out: DEVICE fp32[2] = seg, seg * batch (its contribution to the total).  grad_proto null: value only.  Otherwise grad_coef[l] (fp32, pitch
 * ld_grad_coef[l], a multiple of 4; channels 0..31 of EVERY row written on every call, zeros for a background anchor) and grad_proto (fp32
 * NHWC (batch, mh, mw, 32), pitch ld_grad_proto; every pixel written) hold d (seg * batch) / d input.  No atomics: two calls on the same inputs
 * give the same bits.  topk: dy_detection_loss's (an image has at most gmax * topk foreground anchors).  Nothing synchronises the host; the
 * launch sequence can be captured into a hipGraph. */
#define DY_MASK_U8 0
#define DY_MASK_I32 1
typedef struct dy_seg_loss_desc {
  const int32_t* owner;
  const float* gt;
  const float* coef[DY_MAX_LEVELS];
  int32_t h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld_coef[DY_MAX_LEVELS];
  int32_t n_levels, batch, nm, gmax, topk;
  const void* proto;
  int32_t proto_dtype, ld_proto, mh, mw;
  const void* masks;
  int32_t mask_dtype, gh, gw;
  float img_h, img_w, box_gain;
  float* out;
  void* workspace;
  int64_t workspace_bytes;
  float* grad_coef[DY_MAX_LEVELS];
  int32_t ld_grad_coef[DY_MAX_LEVELS];
  float* grad_proto;
  int32_t ld_grad_proto;
} dy_seg_loss_desc;
int64_t dy_seg_loss_workspace_bytes(int32_t batch, int32_t anchors, int32_t gmax, int32_t topk);
int32_t dy_seg_loss(const dy_seg_loss_desc* d, dy_stream_t stream);
/* dy_space_to_depth2_nhwc: the inverse of dy_depth_to_space2_nhwc (below), for the backward of Proto's transposed convolution:
 * src (n, 2h, 2w, c) -> dst (n, h, w, 4c), dst[n, y, x, (a * 2 + b) * c + o] = src[n, 2y + a, 2x + b, o].  Same dtypes, alignment and c % 8 rule.
 * dy_grad_cast_scaled: fp32 rows (rows, c) of pitch ld_g (a multiple of 4, 16-byte aligned) -> rows of `dtype` (DY_BF16 / DY_F16 / DY_F32; pitch
 * ld_dz, whole 16-byte chunks) = g * (*scale, a DEVICE fp32 value, or 1 when scale is null); c % 8 != 0: DY_ERR_UNSUPPORTED.  It turns
 * dy_seg_loss's gradient maps into the dz of the convolution gradients and applies the deferred seed of the backward pass. */
int32_t dy_space_to_depth2_nhwc(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_src, int32_t ld_dst,
                                int32_t dtype, dy_stream_t stream);
int32_t dy_grad_cast_scaled(const float* g, int32_t ld_g, int64_t rows, int32_t c, const float* scale, void* dz, int32_t ld_dz, int32_t dtype,
                            dy_stream_t stream);

/* ---- convolution gradients ------------------------------------------------------------------
 * Replaces: autograd of F.conv2d inside Conv / RepVGGBlock / Detect (nn/modules/conv.py:37-55) during
 * loss.backward() (engine/trainer.py:381-389).
 * Weight gradient: dw[co][(r*ksize + q)][ci] += sum over output pixels m of dz[m][co] * x[pixel(m) + tap (r,q)][ci].
 *   d describes the FORWARD convolution (x, batch, h, w_in, cin, ld_x, ho, wo, cout, ksize, stride, pad, dtype; w / bias /
 *   y are ignored); dz: NHWC view (batch, ho, wo, cout) of `dtype`, pitch ld_dz; dw: fp32, cout*ksize*ksize*cin, ZEROED by
 *   the caller (partial sums of pixel slabs are added with fp32 atomics).  ld_x / ld_dz must cover cin / cout rounded up to one
 *   16-byte chunk: the padding is read but only reaches entries that are never written, so those elements need be neither zero nor
 *   finite — the product is an outer product over channels summed over PIXELS, and a pad channel of x (dz) is a column (row) of dw
 *   that is dropped; NaN there leaves every written entry as it is (tests/test_view_containment_gpu.py, the "tails" cases: the 3x3,
 *   1x1, generic and image-stem kernels).
 * Input gradient: dx = conv_transpose(dz, w) is run through dy_conv2d_nhwc itself on re-packed weights
 *   (w'[ci][2-r][2-q][co] = w[co][r][q][ci], stride 1; stride-2 layers read dz through `dil2`, a zero-dilated gather).
 * dy_colsum: out[c] += sum over rows of z[row][c] (bias gradient of the plain Detect convolutions); out zeroed by the caller;
 *   z 16-byte aligned, pitch a multiple of 16 bytes covering c rounded up to one chunk: the tail of the last chunk is read, but only
 *   channels < c are summed, so it may hold anything, NaN included. */
int32_t dy_conv2d_wgrad_nhwc(const dy_conv_desc* d, const void* dz, int32_t ld_dz, float* dw, dy_stream_t stream);
/* The same with a caller-owned workspace (device memory, 16-byte aligned, at least dy_conv2d_wgrad_workspace_bytes(d, ld_dz) bytes;
 * NULL / too small: the call behaves as dy_conv2d_wgrad_nhwc).  The 3x3 kernel (16-bit storage) then STORES each pixel slab's partial
 * sums in the workspace and a second launch adds them to dw (1/16 of the atomics: 30-50 us less per layer at batch 64).  Calls that
 * share a workspace must be ordered on one stream.  dy_conv2d_wgrad_workspace_bytes: 0 when the call would not use one; < 0 = dy_status. */
int32_t dy_conv2d_wgrad_nhwc_ws(const dy_conv_desc* d, const void* dz, int32_t ld_dz, float* dw, void* workspace, int64_t workspace_bytes,
                                dy_stream_t stream);
int64_t dy_conv2d_wgrad_workspace_bytes(const dy_conv_desc* d, int32_t ld_dz);
int32_t dy_colsum(const void* z, float* out, int64_t rows, int32_t c, int32_t ld, int32_t dtype, dy_stream_t stream);
/* Grouped convolution (DWConv of yolov8-p2-repvgg-sf.yaml:32,38,44; nn/modules/conv.py:102-107, g = gcd(c1, c2)): both gradients
 * of z = conv2d(x, w, stride, pad, groups) given dz — replaces autograd of F.conv2d for that layer.  d describes the FORWARD
 * convolution (x, batch, h, w_in, cin, ld_x, ho, wo, cout, ksize, stride, pad, groups, dtype).  w_oihw / dw_oihw: the fp32 master
 * weight and its gradient in torch's own (cout, cin/groups, k, k) layout; dw_oihw is ADDED to (zeroed or carrying an earlier
 * micro-batch; fp32 atomics); built for 3x3 kernels with 1, 2 or 4 input channels per group.  dx (optional, with w_oihw): NHWC view
 * (batch, h, w_in, cin) of `dtype`, pitch ld_dx, = conv_transpose(dz, w) (+ dx_accumulate when given).  Either output may be NULL. */
int32_t dy_conv2d_grouped_bwd_nhwc(const dy_conv_desc* d, const void* dz, int32_t ld_dz, const float* w_oihw, float* dw_oihw, void* dx, int32_t ld_dx,
                                   const void* dx_accumulate, int32_t ld_acc, dy_stream_t stream);

/* ---- train-mode BatchNorm2d (+ SiLU) -----------------------------------------------------
 * Replaces: the BatchNorm2d + SiLU half of Conv.forward in training mode (nn/modules/conv.py:37-55; eps 1e-3 and
 * momentum 0.03 are set by initialize_weights, utils/torch_utils.py:423-433) and their autograd backward; the two-branch
 * sum of RepVGGBlock.forward (nn/modules/block.py:1480-1490) through `addend` + dy_silu_fwd / dy_silu_bwd.
 * z: the convolution output, (rows, c) of `dtype`, pitch ld_z (rows = batch*h*w of the NHWC view), c a multiple of one
 * 16-byte chunk and <= 2048 (16-bit) / 1024 (fp32).
 * Forward:  mean/rstd (fp32[c], outputs, saved for backward) = batch statistics of z (biased variance);
 *   y = act(gamma * (z - mean) * rstd + beta (+ addend));  running_mean / running_var (optional) are updated as torch
 *   does: r = (1 - momentum) * r + momentum * stat, the variance unbiased.
 * Backward: dy = gradient w.r.t. y; dz = gradient w.r.t. z; dgamma / dbeta fp32[c] (optional).  With act = SILU the
 *   pre-activation is recomputed from z.  `addend` is not used (its gradient is dy * act'(u): dy_silu_bwd).
 * workspace: dy_bn_workspace_bytes(c) bytes (the 2c sums + one partial per reduction slab), 8-byte aligned.  Sums are
 *   accumulated in double. */
typedef struct dy_bn_desc {
  const void* z;
  void* y;
  const void* addend;
  const void* dy;
  void* dz;
  int64_t rows;
  int32_t c, ld_z, ld_y, ld_add, ld_dy, ld_dz, dtype, act;
  const float* gamma;
  const float* beta;
  float* mean;
  float* rstd;
  float* running_mean;
  float* running_var;
  float eps, momentum;
  float* dgamma;
  float* dbeta;
  void* workspace;
  int64_t workspace_bytes;
  /* > 0 = the workspace ALREADY holds that many partial-sum slots (a convolution epilogue wrote them: dy_conv_desc.bn_stats /
   * dy_conv_stats_written) and the reduction pass is skipped — forward: sums of z and z^2 from the convolution in front;
   * backward: sums of du and du * xhat from the input-gradient convolution behind (dy_conv_desc.bnb_z).  0: the pass runs. */
  int32_t partial_slabs;
} dy_bn_desc;
int64_t dy_bn_workspace_bytes(int32_t c);
int32_t dy_bn_train_fwd(const dy_bn_desc* d, dy_stream_t stream);
int32_t dy_bn_train_bwd(const dy_bn_desc* d, dy_stream_t stream);
/* y = u * sigmoid(u);  du = dy * d/du(u * sigmoid(u)).  (rows, c) views of `dtype`. */
int32_t dy_silu_fwd(const void* u, void* y, int64_t rows, int32_t c, int32_t ld_u, int32_t ld_y, int32_t dtype, dy_stream_t stream);
int32_t dy_silu_bwd(const void* u, const void* dy, void* du, int64_t rows, int32_t c, int32_t ld_u, int32_t ld_dy, int32_t ld_du,
                    int32_t dtype, dy_stream_t stream);

/* ---- small training-path ops -----------------------------------------------------------------
 * dy_upsample2x_bwd_nhwc: gradient of nn.Upsample(None, 2, 'nearest') (yolov8-p2-repvgg.yaml:30,34,38):
 *   dx (n,h,w,c) = sum of the 2x2 blocks of g (n,2h,2w,c).
 * dy_maxpool_bwd_nhwc: gradient of MaxPool2d(k, 1, k//2) inside SPPF (nn/modules/block.py:185-191): every output's
 *   gradient goes to the FIRST maximum of its window in (row, column) order (torch semantics); g_in = (accumulate ?
 *   g_in : 0) + that.  h*w*(52 + 64/elem_size) bytes of LDS per workgroup (16-bit: h*w <= ~1900), k <= 15.
 * dy_add_nhwc: out = a + b, (rows, c) views (Bottleneck's shortcut, block.py:348-350).  c % one 16-byte chunk == 0.
 * dy_add_dilated2_nhwc: dx (n, H2, W2, c)[:, 2y, 2x] += t (n, h, w, c)[:, y, x] -- the input gradient of a 1x1 STRIDE-2 convolution
 *   (RepVGGBlock's 1x1 branch, block.py:1480-1490) from t = the 1x1 stride-1 convolution of dz with the transposed weights.
 * dy_head_grad_split: the gradient of Detect's fp32 training map cat(box, cls) (head.py:69-72; g: (rows, nb + nc) fp32, pitch ld_g) as the
 *   `dtype` operands of the two 1x1 convolutions' gradient kernels in one pass: dzb = s * g[:, :nb]; dzc = s * g[:, nb:nb+nc], zero-padded
 *   to ncp channels; s = *scale (optional DEVICE scalar: the seed loss.backward() starts from, the loss scale under fp16) or 1. */
int32_t dy_upsample2x_bwd_nhwc(const void* g, void* dx, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_g, int32_t ld_dx,
                               int32_t dtype, dy_stream_t stream);
int32_t dy_maxpool_bwd_nhwc(const void* x, const void* g_out, void* g_in, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_x,
                            int32_t ld_go, int32_t ld_gi, int32_t k, int32_t accumulate, int32_t dtype, dy_stream_t stream);
int32_t dy_add_dilated2_nhwc(const void* t, void* dx, int32_t n, int32_t h, int32_t w, int32_t H2, int32_t W2, int32_t c, int32_t ld_t, int32_t ld_dx,
                             int32_t dtype, dy_stream_t stream);
int32_t dy_head_grad_split(const float* g, int32_t ld_g, int64_t rows, int32_t nb, int32_t nc, int32_t ncp, const float* scale, void* dzb, int32_t ld_b,
                           void* dzc, int32_t ld_c, int32_t dtype, dy_stream_t stream);
int32_t dy_add_nhwc(const void* a, const void* b, void* out, int64_t rows, int32_t c, int32_t ld_a, int32_t ld_b, int32_t ld_o,
                    int32_t dtype, dy_stream_t stream);

/* ---- optimizer step, gradient clipping, EMA (flat fp32 tensors) -------------------------------------
 * Replaces: torch.nn.utils.clip_grad_norm_(max_norm 10) + optimizer.step() (engine/trainer.py:591-599) for the SGD
 * (nesterov) / AdamW optimizers build_optimizer creates (trainer.py:764-825: weight decay on the weight group only,
 * so call once per group with its decay), and ModelEMA.update (utils/torch_utils.py:515-545).
 * dy_sumsq_f32: *out += sum g^2 (double; zero it first; call per tensor / bucket, then pass `out` as grad_sumsq).
 * grad_sumsq (optional DEVICE double): total sum of squared gradients; the gradient is scaled by
 *   min(1, max_norm / (sqrt(*grad_sumsq) + 1e-6)) inside the step — no host synchronisation.
 * dy_sgd_step:   g = clip*grad + wd*p;  buf = first_step ? g : momentum*buf + g;  p -= lr * (nesterov ? g + momentum*buf : buf).
 * dy_adamw_step: p *= 1 - lr*wd;  m,v = moments of clip*grad;  p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps); step >= 1.
 * amp_state (optional DEVICE float[4], needs grad_sumsq): the state of torch.cuda.amp.GradScaler (engine/trainer.py:271 `GradScaler`, :389
 *   `scaler.scale(loss).backward()`, :593-596 `unscale_` / `step` / `update`) for fp16 storage — {scale, growth tracker, found_inf of
 *   the last step, skipped steps}.  With it the step kernels divide the gradient by the scale (`unscale_`; the clip norm becomes
 *   sqrt(*grad_sumsq) / scale) and leave p / buf / m / v untouched when *grad_sumsq is not finite (`scaler.step` skips);
 *   AdamW's bias correction counts only the steps that ran.  The caller multiplies the loss gradient by amp_state[0] on the device.
 * dy_amp_update: `scaler.update()` — found_inf: scale *= backoff, tracker = 0, skipped += 1; else tracker += 1 and, every
 *   growth_interval clean steps, scale *= growth (torch defaults: 65536 initial, 2, 0.5, 2000).  Call after the step kernels.
 * dy_ema_update: ema = decay*ema + (1-decay)*p.
 * dy_grad_sink_flush: grad += sink (then sink = 0) for every parameter in ONE launch, where `sink` holds what the backward
 *   kernels produced this batch at the parameter's offset in the flat buffers: weight gradients of dy_conv2d_wgrad_nhwc in
 *   ITS layout (cout, k, k, cin), BatchNorm / bias gradients as they are.  Replaces what autograd's AccumulateGrad does per
 *   parameter (engine/trainer.py:381-389 `loss.backward()`: `param.grad += new`, here ~240 element-wise launches and the
 *   zero-fills of as many temporaries per step).  entries (device, n_entries x 4 int64): {offset, cout, cin, kk}; kk > 1: the
 *   block [offset, offset + cout*cin*kk) of `grad` is (cout, cin, k, k) = torch's layout, of `sink` (cout, k, k, cin);
 *   kk <= 1: plain vector of cout*cin elements. */
int32_t dy_sumsq_f32(const float* g, int64_t n, double* out, dy_stream_t stream);
int32_t dy_sgd_step(float* p, const float* grad, float* buf, int64_t n, float lr, float momentum, float weight_decay, int32_t nesterov,
                    int32_t first_step, const double* grad_sumsq, float max_norm, const float* amp_state, dy_stream_t stream);
int32_t dy_adamw_step(float* p, const float* grad, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int32_t step, const double* grad_sumsq, float max_norm, const float* amp_state, dy_stream_t stream);
int32_t dy_amp_update(float* amp_state, const double* grad_sumsq, float growth_factor, float backoff_factor, int32_t growth_interval, dy_stream_t stream);
int32_t dy_ema_update(float* ema, const float* p, int64_t n, float decay, dy_stream_t stream);
int32_t dy_grad_sink_flush(const int64_t* entries, int32_t n_entries, float* grad, float* sink, dy_stream_t stream);

/* ---- training augmentation on the device (Mosaic + RandomPerspective + RandomHSV + RandomFlip, ultralytics/data/augment.py:490-864,
 * 952-1300, 1303-1390, 1392-1483) -----------------------------------------------------------------
 * dy_augment_u8_nchw: uint8 source images (n_src_imgs, 3, hs, ws) (channel 0 = R) -> ONE augmented uint8 NCHW batch (batch, 3, s, s),
 * what dy_stem_conv3x3s2_nchw_u8 reads.  `table` (DEVICE, one dy_aug_row per output image) holds what the host drew:
 *   n_src = 4: the rectangles of Mosaic._mosaic4 (augment.py:684-708) -- src[i].index's pixels [y1b.., x1b..] pasted at
 *              [y1a:y2a, x1a:x2a] of a ch x cw canvas filled with 114;  n_src = 1: one image on its canvas (the LetterBox pre_transform);
 *   minv:      inverse of M = T S R P C (RandomPerspective.affine_transform, augment.py:1041-1071), row-major, output pixel -> canvas;
 *   hsv:       the three offsets r of RandomHSV.__call__ (augment.py:1379-1384); flags: DY_AUG_FLIPLR | DY_AUG_FLIPUD | DY_AUG_HSV_OFF.
 * Per output pixel: undo the flips, (u, v) = minv (x, y, 1) with the perspective divide, the four bilinear neighbours ON THE CANVAS (a
 * neighbour is the pixel of the source rectangle that covers it, else 114; outside the canvas 114 = borderValue), blended in fp32, rounded
 * to nearest; then RGB -> (H in [0,180), S, V in [0,255]) rounded to integers, H' = trunc((H + r0) mod 180), S' = S ? trunc(clip(S + r1, 0,
 * 255)) : 0, V' = trunc(clip(V + r2, 0, 255)), back to RGB, rounded.  The canvas is never materialised.  s % 4 == 0 (one thread writes four
 * pixels of a plane as one 32-bit word).  A row whose n_src is not 1 or 4, or a source whose index is outside [0, n_src_imgs) or whose
 * pixel lies outside hs x ws, reads nothing and yields 114 there. */
#define DY_AUG_FLIPLR 1
#define DY_AUG_FLIPUD 2
#define DY_AUG_HSV_OFF 4
typedef struct dy_aug_src {
  int32_t index;              /* image of the source tensor */
  int32_t x1a, y1a, x2a, y2a; /* destination rectangle on the canvas (exclusive end) */
  int32_t x1b, y1b;           /* source pixel that lands on (x1a, y1a) */
  int32_t reserved;
} dy_aug_src;
typedef struct dy_aug_row {
  int32_t n_src, ch, cw, flags;
  dy_aug_src src[4];
  float minv[9];
  float hsv[3];
} dy_aug_row;
int32_t dy_augment_u8_nchw(const uint8_t* src, const dy_aug_row* table, uint8_t* dst, int32_t n_src_imgs, int32_t hs, int32_t ws, int32_t batch,
                           int32_t s, dy_stream_t stream);

/* ---- multi-object tracking on the padded NMS output: ByteTrack ----------------------------------------------
 * Replaces: BYTETracker.update (trackers/byte_tracker.py:293-405) with STrack, KalmanFilterXYAH (trackers/utils/kalman_filter.py:65-236),
 * iou_distance / fuse_score / linear_assignment (trackers/utils/matching.py) and the per-image rules of on_predict_postprocess_end
 * (trackers/track.py:71-88), for `streams` independent video streams and `frames` time steps in ONE launch behind dy_nms + dy_scale_boxes;
 * no host synchronisation.  One workgroup per stream walks its time steps in order.
 * rows: fp32 (frames * streams, max_det, 6) x1, y1, x2, y2, conf, cls in source-frame pixels and counts: int32 (frames * streams): what
 * result.boxes holds in the reference; image k is stream k % streams at time step k / streams.  An image with count 0 does not reach the
 * tracker: its stream's frame counter stands still and its output count is 0.
 * state: dy_track_state_bytes(streams, max_tracks) bytes, 16-byte aligned, kept by the caller between calls; dy_track_reset (or zero
 * bytes) = no tracks, frame and id counters 0.  Per stream: int32 frame counter, id counter, overflow counter (first 12 of 64 header
 * bytes), then per slot mean[8] and covariance[8][8] in float64 ([component][slot]) and int32 state (0 free, 1 tracked, 2 lost,
 * 3 removed and waiting out its last update), is_activated, mean-still-float32, id-in-removed-list, id, detection idx, frame_id,
 * start_frame, tracklet_len, then fp32 score and cls.  max_tracks slots hold tracked, lost and unconfirmed tracks together; when they are
 * full, new tracks are not started and the overflow counter grows by the number left out.  max_tracks even, <= 1024; max_det <= 1024;
 * 92 bytes of LDS per slot and 68 per detection (160 KB at most).
 * workspace: dy_track_workspace_bytes(streams, max_tracks, max_det) bytes, 16-byte aligned (the image's measurements; costs are not stored).
 * out: fp32 (frames * streams, max_tracks, 8) x1, y1, x2, y2, id, score, cls, idx = STrack.result of the activated tracked tracks of each
 * step in ASCENDING TRACK ID (the reference emits its Python list order), rows >= out_count zero; out_count: int32 (frames * streams).
 * Ids count from 1 per stream.  The second association's limit 0.5, the unconfirmed one's 0.7 and the duplicate distance 0.15 are the
 * reference's constants.  max_time_lost = int(frame_rate / 30 * track_buffer).
 * The assignments are solved exactly (shortest augmenting paths, float64 potentials); among equal optima the choice is not the
 * reference's (lap's is not defined either). */
typedef struct dy_track_desc {
  const float* rows;
  const int32_t* counts;
  void* state;
  int64_t state_bytes;
  void* workspace;
  int64_t workspace_bytes;
  float* out;
  int32_t* out_count;
  int32_t frames, streams, max_det, max_tracks;
  float track_high_thresh, track_low_thresh, new_track_thresh, match_thresh;
  int32_t fuse_score, max_time_lost;
} dy_track_desc;
int64_t dy_track_state_bytes(int32_t streams, int32_t max_tracks);
int64_t dy_track_workspace_bytes(int32_t streams, int32_t max_tracks, int32_t max_det);
int32_t dy_track_reset(void* state, int32_t streams, int32_t max_tracks, dy_stream_t stream);
int32_t dy_track_step(const dy_track_desc* d, dy_stream_t stream);

/* The same track step for the rows of an oriented-box model (trackers/track.py:69-88 `is_obb`; byte_tracker.py:68-79, :217-228;
 * matching.py:85-94): the second instantiation of the one kernel.  The Kalman filter stays on (x, y, aspect, h); every cost (the three
 * associations and remove_duplicate_stracks) is 1 - ProbIoU(track, detection) on xywha rows rounded to fp32 -- the expression dy_nms_rotated,
 * dy_val_match_rotated and dy_tile_merge_rotated share -- with fuse_score on top as above; the angle is not filtered: a track holds the
 * angle of the detection it last matched.  A NaN in a box or an angle makes its costs NaN = no edge.
 * dy_track_step_rotated takes the same dy_track_desc with these conventions:
 *   rows: fp32 (frames * streams, max_det, 7) x, y, w, h, r, conf, cls (what dy_nms_rotated + dy_scale_rboxes leave);
 *   out:  fp32 (frames * streams, max_tracks, 9) x, y, w, h, r, id, score, cls, idx = STrack.result, ascending track id, rows >= out_count zero.
 * state: dy_track_state_bytes_rotated bytes; the layout above with a third fp32 field per slot behind score and cls: the angle.  All zero =
 * empty as above; dy_track_reset_rotated zeroes this (larger) state.  workspace: dy_track_workspace_bytes_rotated (the measurements again).
 * LDS: 100 bytes per slot (the 92 above + the fifth covariance term and the angle) and 72 per detection (68 + the fifth term); the
 * covariance terms of a box are computed once per slot and once per detection per image.  max_tracks even, <= 1024, max_det <= 1024 AND
 * max_tracks * 100 + max_det * 72 + 64 <= 160 KB: 1024 slots admit 852 detections, the defaults 512 / 300 need 72 864 bytes; a pair beyond
 * that is DY_ERR_INVALID_ARG before any launch, both numbers named. */
int64_t dy_track_state_bytes_rotated(int32_t streams, int32_t max_tracks);
int64_t dy_track_workspace_bytes_rotated(int32_t streams, int32_t max_tracks, int32_t max_det);
int32_t dy_track_reset_rotated(void* state, int32_t streams, int32_t max_tracks, dy_stream_t stream);
int32_t dy_track_step_rotated(const dy_track_desc* d, dy_stream_t stream);

/* ---- instance segmentation: Proto's transposed convolution, the mask-coefficient gather, mask assembly ---------------------
 * dy_depth_to_space2_nhwc: the layout half of nn.ConvTranspose2d(c, c, 2, 2, 0) inside Proto (nn/modules/block.py:80-97).  A k = 2,
 * s = 2, p = 0 transposed convolution is a 1x1 convolution cin -> 4 * cout (GEMM row (a * 2 + b) * cout + o = W[:, o, a, b], the bias
 * repeated four times; dy_conv2d_nhwc) followed by this permutation: src (n, h, w, 4c) -> dst (n, 2h, 2w, c),
 *   dst[n, 2y + a, 2x + b, o] = src[n, y, x, (a * 2 + b) * c + o].
 * A pure move of 16-byte chunks, so it serves DY_BF16 / DY_F16 / DY_F32 / DY_F16X2 alike (DY_FP8: DY_ERR_INVALID_ARG); c % 8 != 0:
 * DY_ERR_UNSUPPORTED.  Pitches in elements, views 16-byte aligned. */
int32_t dy_depth_to_space2_nhwc(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_src, int32_t ld_dst,
                                int32_t dtype, dy_stream_t stream);

/* dy_mask_gather: behind dy_nms and IN FRONT of dy_scale_boxes (ops.process_mask crops with the boxes in input-image pixels,
 * models/yolo/segment/predict.py:66-74).  For every kept row r < counts[b] of image b: out[b, r, 0:4] = rows[b, r, 0:4] and
 * out[b, r, 4:4+nm] = the nm mask coefficients of anchor index[b, r] — what `pred[:, 6:]` holds in the reference after
 * non_max_suppression(nc=...) (utils/ops.py:181-332).  Two sources: per-level fp32 NHWC buffers level[i] (batch, h[i], w[i], nm) with pitch
 * ld[i] (the outputs of Segment.cv4[i], nn/modules/head.py:175-197; anchors are numbered level by level, row-major), or — pred != NULL —
 * a (batch, pred_ch, anchors) fp32 prediction tensor whose channels pred_c0 .. pred_c0 + nm - 1 are the coefficients.  Rows >= counts[b]
 * are neither read nor written; an index outside [0, anchors) writes zeros.  nm != 32: DY_ERR_UNSUPPORTED. */
typedef struct dy_mask_gather_desc {
  const float* rows;      /* (batch, max_det, 6) dy_nms out, unscaled */
  const int32_t* counts;  /* (batch) */
  const int32_t* index;   /* (batch, max_det) dy_nms out_index */
  const float* level[DY_MAX_LEVELS];
  int32_t h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS];
  int32_t n_levels;
  const float* pred;
  int32_t pred_ch, pred_c0, anchors;
  int32_t batch, max_det, nm;
  float* out; /* (batch, max_det, 4 + nm) */
} dy_mask_gather_desc;
int32_t dy_mask_gather(const dy_mask_gather_desc* d, dy_stream_t stream);

/* dy_process_mask: the masks of a whole batch in one launch.  Replaces ops.process_mask(..., upsample=True) (utils/ops.py:679-709: matmul,
 * crop_mask :660-676, F.interpolate bilinear, gt) and, with crop_at_output, ops.process_mask_native + scale_masks (:712-753): dot product,
 * crop, blend and threshold per output pixel, no (n, mh, mw) intermediate.
 * protos: fp32 NHWC (batch, mh, mw, nm), pitch ld_p, 16-byte aligned.  side: the dy_mask_gather output.  counts (batch); offsets
 * (batch + 1): exclusive prefix of counts — detection t of the output belongs to the image b with offsets[b] <= t < offsets[b + 1], row
 * t - offsets[b]; a t that belongs to no image, or whose row is >= counts[b] or >= max_det, gets a zero mask and reads nothing.
 * window: int32 (batch, 4) top, left, sh, sw per image: the part of the proto grid that is resized (clamped into the grid on the device).
 * out: uint8 (total, oh, ow), 0 / 1, 8-byte aligned; every byte is written.  Per output pixel (y, x) of a detection:
 *   src = (dst + 0.5) * (s / o) - 0.5 clamped at 0, i0 = floor(src), i1 = min(i0 + 1, s - 1)  (PyTorch bilinear, align_corners = False),
 *   corner value v = sum_k coef[k] * proto[top + yy, left + xx, k] in fp32, blend of the four corners, mask = blend > 0.
 * crop_at_output == 0: a corner counts as 0 unless bx1 <= xx < bx2 and by1 <= yy < by2 with (bx, by) = the side buffer's box times
 *   ratio_x / ratio_y (= mw / iw, mh / ih as fp32).  crop_at_output == 1: no corner crop; the mask is also 0 unless x1 <= x < x2 and
 *   y1 <= y < y2 for crop_rows[b, r, 0:4] (fp32 (batch, max_det, 6): the rows after dy_scale_boxes).
 *   In both forms a NaN box corner satisfies no inequality (crop_mask's comparisons): the mask is empty.
 * total == 0 returns DY_OK without a launch.  nm != 32: DY_ERR_UNSUPPORTED. */
typedef struct dy_process_mask_desc {
  const float* protos;
  const float* side;
  const int32_t* counts;
  const int32_t* offsets;
  const int32_t* window;
  const float* crop_rows;
  int32_t batch, max_det, nm, mh, mw, ld_p, oh, ow, total, crop_at_output;
  float ratio_x, ratio_y;
  uint8_t* out;
} dy_process_mask_desc;
int32_t dy_process_mask(const dy_process_mask_desc* d, dy_stream_t stream);

/* dy_val_mask_match: the mask half of the segmentation validator for a whole batch behind dy_nms / dy_mask_gather; no host
 * synchronisation.  Replaces, per image, ops.process_mask(proto, coef, box, shape=imgsz) (upsample = False: coef @ protos, crop_mask with the
 * unscaled box times (mw / in_w, mh / in_h), > 0, at PROTOTYPE resolution; utils/ops.py:679-709), the expansion of the overlap label map
 * to one binary mask per label with its F.interpolate(bilinear) + gt(0.5) to the prototype grid, mask_iou (utils/metrics.py:137-153) and
 * BaseValidator.match_predictions (models/yolo/segment/val.py:164-208).  No mask is stored: the map gives a pixel to at most one label, so
 * the intersections of one prediction with all labels are a histogram of the map values under its mask.
 * protos: fp32 NHWC (batch, mh, mw, nm), pitch ld_p, 16-byte aligned; mh * mw <= 2^24 (integer counts exact in fp32).  side: the
 * dy_mask_gather output (batch, max_det, 4 + nm).  rows / counts: the dy_nms outputs (class in column 5; row order = descending confidence).
 * map: (batch, gh, gw) DY_MAP_U8 or DY_MAP_I32, the reference's overlap form: value k >= 1 = the k-th label of the image, 0 = background,
 * values above the image's label count are background.  (mh, mw) == (gh, gw), or exactly (2 gh, 2 gw): then the map is read at
 * [y >> 1, x >> 1] (the resized, thresholded one-hot masks are the 2 x 2 replication of the map).  Anything else: DY_ERR_INVALID_ARG.
 * tcls: fp32 (n_labels) the batch's label classes, image after image; loff: int32 (batch + 1) DEVICE offsets, the labels of image b are
 * tcls[loff[b] .. loff[b + 1]) in map order (clamped into [0, n_labels] on the device).  l_cap: HOST bound on the labels per image (it sizes
 * inter / area_gt; an image with more uses its first l_cap); l_cap > 1024: DY_ERR_UNSUPPORTED (one 4-byte LDS bin per label).
 * iouv: HOST array of n_iouv (1..16) thresholds, read during the call.  in_w, in_h: the network input size the boxes are in.
 * For kept row d of image b and label l: inter = |pred & gt|, iou = inter / (((area_gt + area_pred) - inter) + 1e-7f), every operation
 * rounded on its own (bit-equal to mask_iou); m(l, d) = iou if tcls[l] == cls[d] (cls[d] counts as 0 with single_cls, as in dy_val_match) else 0; best / biou / tp_m by
 * dy_val_match's rule (ties to the lower label position).
 * tp_m: uint8 (batch, max_det, n_iouv).  best_iou: fp32 (batch, max_det); best_label: int32 (batch, max_det), position in tcls, -1 when
 * the image has no label; area_gt: int32 (batch, l_cap).  These three are REQUIRED: they carry the intermediate results between the
 * launches.  Optional: inter int32 (batch, max_det, l_cap), area_pred int32 (batch, max_det).  Every element of every output is written;
 * rows >= counts[b] get 0 / 0 / -1 and zero counts, labels >= the image's count zero areas. */
#define DY_MAP_U8 0
#define DY_MAP_I32 1
typedef struct dy_val_mask_match_desc {
  const float* protos;
  const float* side;
  const float* rows;
  const int32_t* counts;
  const void* map;
  const float* tcls;
  const int32_t* loff;
  const float* iouv;
  int32_t batch, max_det, nm, mh, mw, ld_p, gh, gw, map_dtype, n_labels, l_cap, n_iouv;
  int32_t in_w, in_h, single_cls;
  uint8_t* tp_m;
  float* best_iou;
  int32_t* best_label;
  int32_t* area_gt;
  int32_t* inter;
  int32_t* area_pred;
} dy_val_mask_match_desc;
int32_t dy_val_mask_match(const dy_val_mask_match_desc* d, dy_stream_t stream);

/* ---- pose estimation: keypoint decode, keypoint rescale, batched person crops (csrc/pose.hip) ------------------------------
 * dy_kpt_decode: Pose.kpts_decode (nn/modules/head.py:274-279, the non-export branch).  level[i]: fp32 NHWC (batch, h[i], w[i], nk) with
 * pitch ld[i] >= nk = nkpt * ndim, the outputs of Pose.cv4[i]; anchors are numbered level by level, row-major.  Per keypoint k of the
 * anchor in cell (col, row) of a level with stride s, every step rounded to fp32:
 *   x = (logit[k * ndim] * 2 + ((col + 0.5) - 0.5)) * s,  y the same with row,  v = sigmoid(logit[k * ndim + 2]) when ndim == 3.
 * Two forms, exactly one of pred_kpt / out set:
 *   dense   pred_kpt: fp32 (batch, nk, anchors), the module-level return;
 *   gather  behind dy_nms: out (batch, max_det, nk); for every kept row r < counts[b]: out[b, r, :] = the keypoints of anchor index[b, r].
 *           Rows >= counts[b] are neither read nor written; an index outside [0, anchors) writes zeros.
 * ndim outside {2, 3} or nk > 256: DY_ERR_UNSUPPORTED. */
typedef struct dy_kpt_decode_desc {
  const float* level[DY_MAX_LEVELS];
  int32_t h[DY_MAX_LEVELS], w[DY_MAX_LEVELS], ld[DY_MAX_LEVELS];
  float stride[DY_MAX_LEVELS];
  int32_t n_levels;
  int32_t batch, anchors, nkpt, ndim;
  float* pred_kpt;        /* dense form, or NULL */
  const int32_t* counts;  /* gather form: (batch) dy_nms out_count */
  const int32_t* index;   /* (batch, max_det) dy_nms out_index */
  int32_t max_det;
  float* out;             /* (batch, max_det, nk), or NULL */
} dy_kpt_decode_desc;
int32_t dy_kpt_decode(const dy_kpt_decode_desc* d, dy_stream_t stream);

/* dy_scale_coords: PosePredictor.construct_result's ops.scale_coords (models/yolo/pose/predict.py:46-48; utils/ops.py:756-788 with
 * clip_coords :357-374) and the Keypoints constructor's masking (engine/results.py:1373-1375), in place on the gathered rows
 * kpts (batch, max_det, nkpt, ndim) for rows < counts[b].  params: fp32 (batch, 7) gain, pad_x, pad_y, clip_w, clip_h, off_x, off_y; the
 * pads are the UNROUNDED (img1 - img0 * gain) / 2 (scale_boxes rounds them, scale_coords does not).  Per keypoint:
 *   x = min(max((x - pad_x) / gain, 0), clip_w), y the same; then ndim == 3 and v < 0.5: x = y = 0; otherwise x += off_x, y += off_y
 * (the offsets are zero except for crops of a frame).  boxes: NULL, or the dy_nms rows (batch, max_det, 6) AFTER dy_scale_boxes: a
 * non-zero offset is added to x1, y1, x2, y2 of every row < counts[b] as well (a crop's boxes, clamped to the crop, move to frame pixels).
 * ndim outside {2, 3}: DY_ERR_UNSUPPORTED. */
int32_t dy_scale_coords(float* kpts, float* boxes, const int32_t* counts, const float* params, int32_t batch, int32_t max_det, int32_t nkpt,
                        int32_t ndim, dy_stream_t stream);

/* dy_crops_letterbox_u8_to_nchw_f32: the batched person-crop slicer.  frames: DEVICE uint8 (f, hf, wf, 3), all frames one shape.
 * table: DEVICE int32 (k, 9), per crop  frame, x0, y0, cw, ch, new_w, new_h, top, left;  table_host: the same table in HOST memory, read
 * during the call for the argument check.  dst: fp32 (k, 3, hn, wn).  Crop j is the ch x cw window of its frame at (y0, x0), resized to
 * new_h x new_w by the 8-bit bilinear rule of dy_letterbox_u8_to_nchw_f32 (a size equal to the window copies), placed at (top, left),
 * pad_value elsewhere, / 255, swap_rb: bit for bit what dy_letterbox_u8_to_nchw_f32 writes for a contiguous copy of the window.
 * A row whose window leaves the frame, whose cw or ch is < 1 or whose resized image leaves the output: DY_ERR_INVALID_ARG, nothing launched.
 * k <= 65535. */
int32_t dy_crops_letterbox_u8_to_nchw_f32(const uint8_t* frames, const int32_t* table, const int32_t* table_host, float* dst, int32_t f, int32_t hf,
                                          int32_t wf, int32_t k, int32_t hn, int32_t wn, int32_t swap_rb, float pad_value, dy_stream_t stream);

/* ---- pose validation: object keypoint similarity and matching on the padded NMS output (csrc/val_oks.hip) --------------------
 * dy_val_oks_match.  Replaces: PoseValidator._process_batch's keypoint branch (models/yolo/pose/val.py: match_predictions on
 * kpt_iou(gt_kpts, pred_kpts, sigma, area = box area * 0.53), utils/metrics.py:156-175) with the clip of its _prepare_pred
 * (ops.scale_coords at gain 1 / pad 0 = clip_coords), for a whole batch in one launch behind dy_nms; no host synchronisation, no
 * allocation, capturable in a hipGraph.
 * rows: fp32 (batch, max_det, 6) and counts: int32 (batch): the dy_nms outputs; only the class column is read, rows >= counts[b] never.
 * kpts: the predictions' keypoints.  Coordinate c of keypoint k of kept row d of image b is
 *     kpts[b * stride_b + (k * ndim + c) * stride_ch + (index ? index[b * max_det + d] : d) * stride_d]       (strides in floats)
 *   dense plus index  index = dy_nms out_index, stride_b = C * A, stride_ch = A, stride_d = 1 and kpts = pred + (4 + nc) * A read the
 *                     (batch, C, A) tensor the unfused Pose.forward returns; an index outside [0, anchors) is clamped into it;
 *   gathered rows     index = NULL, stride_b = max_det * nk, stride_d = nk, stride_ch = 1: the dy_kpt_decode gather output.
 *   Only c = 0 and 1 are read (a prediction's visibility is not used); rows >= counts[b] are never read in either form.
 * tbox: fp32 (n_labels, 4) label boxes, xyxy in pixels, clipped, 16-byte aligned; tkpt: fp32 (n_labels, nkpt, 3) x, y in pixels, clipped,
 * and visibility; tcls: fp32 (n_labels); timg: int32 (n_labels), any order.  n_labels = 0 with null label pointers is valid.
 * sigma: HOST array of nkpt floats, iouv: HOST array of n_iouv (1..16) thresholds, both read during the call.
 * nkpt in [1, DY_OKS_MAX_KPT] (above: DY_ERR_UNSUPPORTED), ndim 2 or 3, max_det <= 4096.
 * fp32 in kpt_iou's order of operations without contraction:  px = min(max(x, 0), clip_w), py likewise;  per label
 *   area = ((x2 - x1) * (y2 - y1)) * 0.53f,  den[k] = (((2 sigma[k]) * (2 sigma[k])) * (area + 1e-7f)) * 2;  per pair
 *   d[k] = dx * dx + dy * dy,  e[k] = d[k] / den[k] (correctly rounded),  oks = (sum_k expf(-e[k]) * (vis[k] != 0)) / (n_visible + 1e-7f);
 *   m(l, d) = oks if tcls[l] == cls[d] (0 with single_cls) else 0; a label without a visible keypoint scores 0.  expf is the device's
 *   and the sum runs k = 0, 1, ...: not bit-equal to the host's.  best / biou / tp by dy_val_match's rule (ties to the lower position in
 *   tbox, a NaN never becomes the best).
 * tp: uint8 (batch, max_det, n_iouv); best_iou / best_label: optional, as in dy_val_match.  Every element is written; rows >= counts[b]
 * get 0 / 0 / -1.  One workgroup per image; labels per image are unbounded. */
#define DY_OKS_MAX_KPT 32
typedef struct dy_val_oks_match_desc {
  const float* rows;
  const int32_t* counts;
  const float* kpts;
  const int32_t* index; /* (batch, max_det) dy_nms out_index, or NULL */
  int64_t stride_b, stride_ch, stride_d;
  int32_t anchors; /* dense form: the range of index */
  const float* tbox;
  const float* tkpt;
  const float* tcls;
  const int32_t* timg;
  const float* sigma;
  const float* iouv;
  int32_t batch, max_det, n_labels, n_iouv, nkpt, ndim;
  float clip_w, clip_h;
  int32_t single_cls;
  uint8_t* tp;
  float* best_iou;
  int32_t* best_label;
} dy_val_oks_match_desc;
int32_t dy_val_oks_match(const dy_val_oks_match_desc* d, dy_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DYOLO_H_ */
