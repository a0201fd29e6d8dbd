"""Tensor-level wrappers over the libdyolo C-ABI.

Activations are torch tensors that are *logically* (N, C, H, W) — the shape the reference's
modules exchange (nn/tasks.py:148-154) — but live in NHWC memory: ``stride(1) == 1`` and
``stride(3)`` is the pixel pitch ``ld``.  A channel slice ``buf[:, c0:c1]`` of such a tensor is a
valid view for every kernel, which is how Concat / chunk are done without copies.

PyTorch is used here for device memory and streams only; every arithmetic op on the hot path
is a libdyolo kernel.  A ``LaunchPlan`` records the (function, arguments) list of a forward so
later forwards with the same shapes replay the launches without re-running the Python modules.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import os
import warnings

import torch

from . import _lib
from ._lib import DY_ACT_NONE, DY_ACT_SILU, DY_ACT_SILU_L2E, BnDesc, BranchDesc, C2fDesc, C2fFrontDesc, C2fTailDesc, ConvDesc, DecodeDesc, HeadDecodeDesc, LossDesc, NmsDesc, ObbLossDesc, SegLossDesc, Stem2Desc, TileFuseDesc, TileMergeDesc, TrackDesc, ValMaskMatchDesc, ValMatchDesc, check, lib

FP8 = torch.float8_e4m3fn  # OCP e4m3fn: gfx950's fp8 (MI300's fnuz is another encoding)
# DY_F16X2 (include/dyolo.h): split float16 pairs, x ~= hi + lo * 2^-11 — the bar-exact precision on the 16-bit MFMA.  torch has no such
# type; its tensors are carried as torch.complex32 — a 4-byte element of two halves — purely as a CONTAINER: shapes, strides, channel
# slices at multiples of 8 and raw copies mean what they say, arithmetic on them in torch does not (inside a pixel row the halves are
# laid out [hi x 8 | lo x 8] per 8 channels, not interleaved per element).  ``to_nchw_f32`` gives the values back.
F16X2 = torch.complex32
_DTYPES = {torch.bfloat16: _lib.DY_BF16, torch.float16: _lib.DY_F16, torch.float32: _lib.DY_F32, FP8: _lib.DY_FP8, F16X2: _lib.DY_F16X2}
warnings.filterwarnings("ignore", message="ComplexHalf support is experimental")

# DY_FP8: ONE activation scale for the whole network (real value = quantum * scale), per-output-channel weight scales
# (include/dyolo.h, dy_conv_desc.w_scale / act_scale).  Set by the predictor from a calibration pass before any fp8 pack is built.
_FP8 = {"act_scale": 1.0}


def set_fp8_act_scale(scale: float) -> None:
    if not scale > 0:
        raise ValueError("fp8 activation scale must be positive")
    _FP8["act_scale"] = float(scale)


def fp8_act_scale() -> float:
    return _FP8["act_scale"]


_absmax_log: Optional[list] = None  # calibration: conv2d appends the absolute maximum of every output while this is a list


class observe_absmax:
    """Context manager: records max |y| of every conv output launched inside (device scalars; read them after a sync)."""

    def __enter__(self):
        global _absmax_log
        _absmax_log = []
        return _absmax_log

    def __exit__(self, *exc):
        global _absmax_log
        _absmax_log = None
        return False



def dy_dtype(dt: torch.dtype) -> int:
    try:
        return _DTYPES[dt]
    except KeyError:
        raise TypeError(f"unsupported activation dtype {dt}; use bfloat16, float16 or float32") from None


_ESIZE = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4, FP8: 1, F16X2: 4}


def elems_per_chunk(dt: torch.dtype) -> int:
    return 16 // (_ESIZE.get(dt) or torch.empty((), dtype=dt).element_size())


def chan_gran(dt: torch.dtype) -> int:
    """Channels per addressable group of a pixel row: one 16-byte chunk, or — split float16 — a (hi, lo) chunk pair of 8 channels."""
    return 8 if dt == F16X2 else elems_per_chunk(dt)


def require_device(t: torch.Tensor, what: str = "tensor") -> None:
    """The hot path is HIP only: refuse CPU tensors loudly instead of falling back."""
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} is on '{t.device}': the Drone-YOLO hot path runs on an MI355X (HIP) device only; "
            "there is no CPU fallback in this package."
        )


def alloc_nhwc(n: int, c: int, h: int, w: int, dtype: torch.dtype, device, ld: Optional[int] = None) -> torch.Tensor:
    """Logical (n,c,h,w) tensor in NHWC memory with pixel pitch ``ld`` (default c)."""
    ld = c if ld is None else ld
    buf = torch.empty((n, h, w, ld), dtype=dtype, device=device)
    return buf.permute(0, 3, 1, 2)[:, :c]


def view_params(t: torch.Tensor) -> Tuple[int, int]:
    """(data_ptr, ld) of an NHWC view; raises if ``t`` is not one."""
    if t.dim() != 4:
        raise ValueError(f"expected a 4-D (N,C,H,W) tensor, got shape {tuple(t.shape)}")
    n, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    ld = sw if w > 1 else (sh if h > 1 else (sn if n > 1 else c))
    ok = (c == 1 or sc == 1) and (w == 1 or sw == ld) and (h == 1 or sh == w * ld) and (n == 1 or sn == h * w * ld)
    if not ok or ld < c:
        raise ValueError(
            f"tensor of shape {tuple(t.shape)} / strides {t.stride()} is not an NHWC view; "
            "use hip_ops.to_nhwc() or torch.channels_last"
        )
    return t.data_ptr(), ld


# ---- launch plan ------------------------------------------------------------------------------


class LaunchPlan:
    """Recorded kernel launches of one forward: list of (cfunc, args) + the buffers they use."""

    def __init__(self):
        self.ops: List[Tuple[object, tuple, bool]] = []  # (cfunc, args-without-stream, by_desc)
        self.tags: List[object] = []  # per op: the model layer that issued it (``layer_tag``; None outside a layer) — per-layer profiling
        self.keep: List[object] = []  # tensors / descriptors that must outlive the plan
        self.input_slot: Optional[Tuple[int, int]] = None  # (op index, arg index) of the user input pointer
        self.outputs = None

    def replay(self, stream: int, start: int = 0, stop: Optional[int] = None) -> None:
        """Issue the recorded launches (ops[start:stop]) on ``stream``."""
        for fn, args, _ in (self.ops if start == 0 and stop is None else self.ops[start:stop]):
            rc = fn(*args, stream)
            if rc:
                check(rc, fn.__name__)

    def rebind_input(self, ptr: int) -> None:
        i, j = self.input_slot
        fn, args, d = self.ops[i]
        if j < 0:  # the input pointer is field ``x`` of the descriptor passed by reference
            args[0]._obj.x = ptr
            return
        args = list(args)
        args[j] = ptr
        self.ops[i] = (fn, tuple(args), d)


_recording: Optional[LaunchPlan] = None
_LAYER_TAG = [None]  # (index, type name) of the model layer whose forward is running (set by nn/tasks.py::_predict_layers)


class layer_tag:
    """Launches issued inside are attributed to model layer ``tag`` in a recording plan (``LaunchPlan.tags``)."""

    def __init__(self, tag):
        self.tag = tag

    def __enter__(self):
        self.prev, _LAYER_TAG[0] = _LAYER_TAG[0], self.tag

    def __exit__(self, *exc):
        _LAYER_TAG[0] = self.prev
        return False


class record:
    """Context manager: launches issued inside are also appended to ``plan``."""

    def __init__(self, plan: LaunchPlan):
        self.plan = plan

    def __enter__(self):
        global _recording
        if _recording is not None:
            raise RuntimeError("nested LaunchPlan recording")
        _recording = self.plan
        return self.plan

    def __exit__(self, *exc):
        global _recording
        _recording = None
        return False


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _launch(fn, args: tuple, keep: Sequence[object] = (), record: bool = True) -> None:
    """``record=False``: one-time preparation (weight packing) that must not be replayed with a plan recorded around it."""
    rc = fn(*args, _stream())
    if rc:
        check(rc, fn.__name__)
    if _recording is not None and record:
        _recording.ops.append((fn, args, False))
        _recording.tags.append(_LAYER_TAG[0])
        _recording.keep.extend(keep)


# ---- convolution --------------------------------------------------------------------------------


def _zero_padded(t: torch.Tensor, n_elems: int, shape) -> torch.Tensor:
    """``t`` zero-padded at the end of every dim to ``shape``: ``n_elems`` elements (a packed image is sized by its plan)."""
    out = torch.zeros(n_elems, dtype=t.dtype, device=t.device).view(shape)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


def _permute_cast(view: torch.Tensor, dtype: torch.dtype, n_elems: int) -> torch.Tensor:
    """Contiguous copy of a permuted view, ``n_elems`` elements of ``dtype``, flat — one copy kernel for layout change + cast."""
    out = torch.empty(n_elems, dtype=dtype, device=view.device).view(view.shape)
    out.copy_(view)
    return out.view(-1)


_ZERO_BIAS = {}


def zero_bias(n: int, device) -> torch.Tensor:
    """Cached fp32 zeros(n) on ``device`` (BatchNorm-ed and gradient convolutions carry no bias); never written to."""
    key = (n, str(device))
    z = _ZERO_BIAS.get(key)
    if z is None:
        z = _ZERO_BIAS[key] = torch.zeros(n, dtype=torch.float32, device=device)
    return z


# ---- the log2(e)-scaled activation domain (DY_ACT_SILU_L2E, include/dyolo.h) ---------------------------------------------
LOG2E = 1.4426950408889634
_SCALED = [False]


class scaled_activations:
    """While active, weights are packed for a pass whose stored activations are log2(e) times the reference's: every bias times
    log2(e), the weights of a layer that reads raw data (the image) likewise, SiLU as DY_ACT_SILU_L2E (one VALU instruction less per
    output element), the plain 1x1 convolutions that end the Detect branches divided by log2(e) so that the logits come out in true
    units.  Max pool, nearest upsample, Concat and the Bottleneck sum commute with the positive scale.  The model executor
    (nn/tasks.py::_predict_once) turns it on for 16-bit / fp8 storage; modules called on their own stay in the reference's units."""

    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _SCALED[0]
        _SCALED[0] = self.on
        return self

    def __exit__(self, *exc):
        _SCALED[0] = self.prev
        return False


def scaled_domain() -> bool:
    return _SCALED[0]


def domain_fold(w: torch.Tensor, b: torch.Tensor, silu: bool, raw_input: bool = False, raw_output: bool = False):
    """(weight, bias, activation code) of one convolution for the activation domain in force (see ``scaled_activations``)."""
    if not _SCALED[0]:
        return w, b, (DY_ACT_SILU if silu else DY_ACT_NONE)
    w, b = w.detach().float(), b.detach().float()
    if raw_output:
        if silu or raw_input:
            raise ValueError("domain_fold: a layer that leaves the scaled domain is a plain convolution on scaled input")
        return w / LOG2E, b, DY_ACT_NONE
    return (w * LOG2E if raw_input else w), b * LOG2E, (DY_ACT_SILU_L2E if silu else DY_ACT_NONE)


def _act_code(act) -> int:
    return int(act) if isinstance(act, int) and not isinstance(act, bool) else (DY_ACT_SILU if act else DY_ACT_NONE)


class PackCache:
    """Weight packing of a whole training step in one launch.  A step packs every convolution's fp32 master weights twice (forward
    and input-gradient form): ~160 ``dy_pack_conv_weights`` launches of ~5 us.  The first step under ``batched_weight_packing`` packs
    one by one and remembers each job with a PERSISTENT destination; from then on ``pack_all()`` (the trainer calls it at the start of
    a step, i.e. after the optimizer changed the weights) runs all of them as ONE ``dy_pack_conv_weights_batched`` launch and the
    ``PackedConv`` constructors of that step take the packed buffers as they are.  Sources are the flat parameter buffer's views
    (stable addresses); a job that first appears later is packed on its own and joins the table at the next ``pack_all`` outside a
    stream capture (the table is uploaded with a host-to-device copy)."""

    def __init__(self, dtype: torch.dtype, device, stable: torch.Tensor):
        """``stable``: the buffer whose views may be cached (the trainer's flat parameter buffer) -- weights built per step
        (a padded copy, a folded RepVGG kernel) have another address every time and are packed on their own."""
        self.dtype, self.device = dtype, torch.device(device)
        self.lo, self.hi = stable.data_ptr(), stable.data_ptr() + stable.numel() * stable.element_size()
        self.jobs: dict = {}      # job tuple -> [destination, generation packed, keep-alive source]
        self.table = None         # (device table, n_jobs, total_blocks, job order)
        self.dirty = False
        self.gen = 0
        self._retired = []  # superseded job tables (see _build)

    def lookup(self, job):
        e = self.jobs.get(job)
        return e[0] if e is not None and e[1] == self.gen else None

    def slot(self, job, src) -> torch.Tensor:
        e = self.jobs.get(job)
        if e is None:
            e = self.jobs[job] = [torch.empty(job[11], dtype=self.dtype, device=self.device), -1, src]
            self.dirty = True
        e[1] = self.gen  # the caller packs it now
        return e[0]

    def _build(self) -> None:
        L = lib()
        order = list(self.jobs)
        n = len(order)
        arr = (_lib.PackJob * n)()
        for i, j in enumerate(order):
            a = arr[i]
            a.w, a.s_co, a.s_ci, a.s_r, a.s_q, a.cout, a.cin, a.ksize, a.transpose_flip, a.cin_logical, a.w_layout = j[:11]
            a.dst, a.dst_elems = self.jobs[j][0].data_ptr(), j[11]
        nbytes = int(L.dy_pack_conv_weights_table_bytes(n))
        host = torch.empty(nbytes, dtype=torch.uint8)
        blocks = C.c_int32(0)
        check(L.dy_pack_conv_weights_table(arr, n, dy_dtype(self.dtype), host.data_ptr(), nbytes, C.byref(blocks)), "dy_pack_conv_weights_table")
        if self.table is not None:
            # a captured step graph has the old table's device address baked into its dy_pack_conv_weights_batched node: a table that
            # was ever launched stays allocated for the life of the cache (a few KB each; rebuilt only when a new layer shape appears)
            self._retired.append(self.table[0])
        self.table = (host.to(self.device), n, int(blocks.value), order)
        self.dirty = False

    def pack_all(self) -> None:
        """Start of a step: everything known is packed again from the current weights."""
        if not self.jobs:
            return
        if (self.dirty or self.table is None) and not torch.cuda.is_current_stream_capturing():
            self._build()
        self.gen += 1
        if self.table is None:
            return
        tab, n, blocks, order = self.table
        _launch(lib().dy_pack_conv_weights_batched, (tab.data_ptr(), n, blocks, dy_dtype(self.dtype)), record=False)
        for j in order:
            self.jobs[j][1] = self.gen


_PACK_CACHE = {"active": None}
HREG_128 = [os.environ.get("DYOLO_HREG_128", "1") != "0"]  # see conv_pack_plan: 128-channel 3x3 layers on the register-weight kernel (0: the virtual-flat GEMM, for A/B runs)
FLAT_K_3X3 = [os.environ.get("DYOLO_FLAT_K_3X3", "1") != "0"]  # see conv_pack_plan: odd-width 3x3 layers on the flat-K kernel (0: the halo kernel, for A/B runs)


@contextlib.contextmanager
def batched_weight_packing(cache: Optional[PackCache]):
    """``PackedConv`` constructions of device-resident fp32 weights inside this block go through ``cache`` (see PackCache)."""
    prev = _PACK_CACHE["active"]
    _PACK_CACHE["active"] = cache
    try:
        yield cache
    finally:
        _PACK_CACHE["active"] = prev


class ConvPackPlan(NamedTuple):
    """What ``conv_pack_plan`` decides for one convolution: the weight layout and the geometry of the packed image."""
    layout: int   # DY_WLAYOUT_* (include/dyolo.h)
    cin: int      # logical input channels (zero-padded ones included)
    k_pad: int    # DY_WLAYOUT_ROWS: elements per row; 0 in the fragment layouts
    cout_pad: int  # entries of the padded bias (and rows of a DY_WLAYOUT_ROWS image)
    groups: int
    e: int        # elements per 16-byte chunk; the tile geometry below is 0 in DY_WLAYOUT_ROWS
    kc: int       # input channels per K chunk (4 * e)
    bn: int       # output channels per tile
    nt: int       # cout tiles
    nch: int      # K chunks (HALO3X3) / K groups (FRAG1X1) of kc channels
    n_elems: int  # elements of the packed image, in the storage type


def _frag1x1_plan(cout: int, cin: int, dtype: torch.dtype, cout_pad: int = 0) -> ConvPackPlan:
    """DY_WLAYOUT_FRAG1X1 geometry: the tile width follows from cout alone; the bias covers whole tiles (and ``cout_pad`` at least)."""
    e = elems_per_chunk(dtype)
    kc, bn = 4 * e, (128 if cout > 64 else (64 if cout > 16 else 16))
    nt, nkg = -(-cout // bn), -(-cin // kc)
    return ConvPackPlan(_lib.DY_WLAYOUT_FRAG1X1, cin, 0, max(cout_pad, nt * bn), 1, e, kc, bn, nt, nkg, nt * nkg * (bn // 16) * 64 * e)


def conv_pack_plan(cout: int, cin: int, k: int, stride: int, pad: int, groups: int, act_code: int, dtype: torch.dtype,
                   halo: Optional[bool] = None, for_out_f32: bool = False) -> ConvPackPlan:
    """This shape -> this weight layout, this geometry: the one place that decides which kernel family a convolution is packed for.
    Integers and flags only.  ``cin``: the logical input channels — after ``cin_pad``, and for dense split float16 rounded up to 8;
    ``halo`` / ``for_out_f32``: as for ``PackedConv``.  Host and device packers both size their image by ``n_elems``."""
    if groups != 1:
        if dtype == F16X2 and (cout != groups or cin // groups not in (1, 2, 4) or cout % 8):
            # DWConv of the -sf YAML: the small-group kernel multiplies joined fp32 inputs by fp32 weights (rows [cout][taps][cin / groups])
            raise NotImplementedError("split-float16 storage of a grouped convolution: one output channel per group, 1 / 2 / 4 inputs each, cout % 8 == 0")
        if dtype == FP8:
            raise NotImplementedError("fp8 storage is built for dense convolutions")
        k_pad = k * k * (cin // groups)  # grouped rows carry no padding
        return ConvPackPlan(_lib.DY_WLAYOUT_ROWS, cin, k_pad, cout, groups, 0, 0, 0, 0, 0, cout * k_pad)
    L = lib()
    k_pad, cout_pad = L.dy_conv_k_pad(cin, k, dy_dtype(dtype)), L.dy_conv_cout_pad(cout)
    rows = ConvPackPlan(_lib.DY_WLAYOUT_ROWS, cin, k_pad, cout_pad, 1, 0, 0, 0, 0, 0, cout_pad * k_pad)
    if dtype in (F16X2, FP8):  # rows layout only
        return rows
    # stride-2 halo tiles are 17x33 pixels (2 x 45 KB of LDS): only a weight set of <= 36 KB fits beside them
    s2_fits = cin <= 4 * elems_per_chunk(dtype) and cout > 32 or cin <= 8 * elems_per_chunk(dtype) and cout <= 32
    # r03: the 64-channel downsampling layers run on the register-weight stride-2 kernel (conv3x3_hreg_s2), same fragment layout
    s2_fits = s2_fits or (dtype in (torch.bfloat16, torch.float16) and cin == 64 and cout % 64 == 0 and cout <= 256 and halo is not False)
    # deep 3x3 layers (small maps, weight sets far beyond LDS) run faster as a flat-M implicit GEMM on the LDS-DMA
    # big-tile kernel behind DY_WLAYOUT_ROWS (conv_gemm_glds.hip): measured at batch 128, 256->256 @20x20 90 vs 162 us
    kstep = 8 * elems_per_chunk(dtype)
    # r04: 128 input channels fit the register-weight kernel too (four 32-channel chunks: 144 weight registers, two workgroups per CU):
    # 128->128 @40x40 149 -> 136 us, @80x80 543 -> 437 us (1,100 TFLOP/s) at B = 256 against the virtual-flat GEMM
    # r05: bf16 INFERENCE packs stay on the virtual-flat GEMM: the four-chunk summation order moved the s640 fixture's worst bf16 box from
    # IoU 0.9981 to 0.9979, under the 0.998 floor of tests/test_model_gpu.py, and the floor is not what gives way; fp16 -- the
    # 16-bit inference dtype, 8x finer -- did not move, and the raw convolutions of a training step (no activation: BatchNorm follows) keep
    # the kernel for its statistics epilogue
    hreg128 = HREG_128[0] and halo is None and k == 3 and stride == 1 and pad == 1 and groups == 1 and \
        (dtype == torch.float16 or (dtype == torch.bfloat16 and act_code == 0)) and cin == 128 and cout % 64 == 0 and cout <= 256
    deep3x3 = halo is None and k == 3 and stride == 1 and cin % kstep == 0 and cout % 64 == 0 and \
        cin >= 128 and cout >= 128 and not hreg128
    # (r04: deep layers whose cout is no multiple of 128 — scale x: 320 -> 320 — take the flat-K kernel's 160-wide tiles behind the same
    # layout (csrc/conv_igemm.hip: fk_first): 19.09 -> 18.68 ms per x1536 pass against the halo kernel, 536 -> 860 TFLOP/s against the
    # 64-cout persistent tiles of the tap-aligned kernel)
    # r04: 3x3 layers whose channel counts are not whole 64-channel K-steps / 64-cout tiles (the n / m / x scales: 80, 160, 320 ...)
    # run on the flat-K LDS-DMA kernel behind DY_WLAYOUT_ROWS (conv_gemm_fk.hip) instead of the halo kernel's 32-channel chunks
    flat3x3 = FLAT_K_3X3[0] and halo is None and k == 3 and pad == 1 and groups == 1 and dtype in (torch.bfloat16, torch.float16) and \
        cin >= 64 and (cin % 64 != 0 or cout % 64 != 0) and cin % 8 == 0 and cout % 8 == 0
    if (halo is None or halo) and not deep3x3 and not flat3x3 and groups == 1 and k == 3 and pad == 1 and (stride == 1 or (stride == 2 and s2_fits)) \
            and cout % 4 == 0 and cin >= 4 * elems_per_chunk(dtype) // 2:
        # LDS-halo 3x3 kernel: MFMA-fragment-ordered weights (include/dyolo.h, DY_WLAYOUT_HALO3X3)
        e = elems_per_chunk(dtype)
        kc, bn = 4 * e, (64 if cout > 32 else 32)
        nt, nch = -(-cout // bn), -(-cin // kc)
        return ConvPackPlan(_lib.DY_WLAYOUT_HALO3X3, cin, 0, cout_pad, 1, e, kc, bn, nt, nch, nt * nch * 9 * (bn // 16) * 64 * e)
    if (halo is None or halo) and groups == 1 and k == 1 and stride == 1 and pad == 0 and L.dy_conv1x1_stream_supported(cin, cout, dy_dtype(dtype), for_out_f32):
        # streaming 1x1 kernel: fragment-ordered weights, single tap (include/dyolo.h, DY_WLAYOUT_FRAG1X1)
        return _frag1x1_plan(cout, cin, dtype, cout_pad)
    return rows


def _split_f16x2(rows: torch.Tensor):
    """The split-float16 rule (include/dyolo.h, DY_F16X2), (hi, lo, inverse row scale) of fp32 ``rows``: every row (dim 0) times the power
    of two that puts its largest weight in [2^13, 2^14) (exact; the inverse goes to w_scale and multiplies the accumulator), then
    hi = rn_f16(w) — 0 below float16's smallest normal — and lo = rn_f16(w - hi), UNSCALED: the kernel multiplies x_hi by it directly and
    forms w_hi 2^-11 for the x_lo term itself."""
    amax = rows.abs().amax(tuple(range(1, rows.dim()))).clamp_min(1e-30)
    sc = torch.exp2(13.0 - torch.floor(torch.log2(amax)))
    ws = rows * sc.view(-1, *([1] * (rows.dim() - 1)))
    hi = torch.where(ws.abs() < 2.0 ** -14, torch.zeros_like(ws), ws).to(torch.float16)
    lo = (ws - hi.to(torch.float32)).to(torch.float16)
    return hi, lo, 1.0 / sc


def _padded_bias(bias: torch.Tensor, n: int, device) -> torch.Tensor:
    """fp32 ``bias`` zero-padded to ``n`` entries on ``device``.  A training step must not pay a fill + copy per convolution: a bias that
    already is fp32 on the GPU at that length is used as it is, the shared zeros (``zero_bias``: training, gradient convolutions) stay
    the shared zeros."""
    if bias.numel() == n and bias.is_cuda and bias.dtype == torch.float32:
        return bias.detach()
    if bias is _ZERO_BIAS.get((bias.numel(), str(device))):
        return zero_bias(n, device)
    bp = torch.zeros((n,), dtype=torch.float32, device=device)
    bp[: bias.numel()] = bias.detach().to(torch.float32).to(device)
    return bp


def _rows_image(weight: torch.Tensor, plan: ConvPackPlan, dtype: torch.dtype) -> torch.Tensor:
    """DY_WLAYOUT_ROWS in a plain storage type: (cout, k, k, cin / groups) rows, zero padded to (cout_pad, k_pad)."""
    if plan.groups == 1 and plan.n_elems == weight.numel():  # nothing to pad: one permute + cast kernel
        return _permute_cast(weight.permute(0, 2, 3, 1), dtype, plan.n_elems)
    rows = weight.to(torch.float32).permute(0, 2, 3, 1).reshape(weight.shape[0], -1)
    if plan.n_elems != rows.numel():  # (grouped rows carry no padding)
        rows = _zero_padded(rows, plan.n_elems, (plan.cout_pad, plan.k_pad))
    return rows.to(dtype).contiguous()


def _rows_image_fp8(weight: torch.Tensor, plan: ConvPackPlan, act_scale: float):
    """DY_WLAYOUT_ROWS in e4m3 with one scale per OUTPUT channel (absmax -> 448): (image, scales); the epilogue multiplies the
    accumulator by act_scale * weight_scale[co] (include/dyolo.h)."""
    cout = weight.shape[0]
    rows = weight.to(torch.float32).permute(0, 2, 3, 1).reshape(cout, -1)
    ws = (rows.abs().amax(1) / 448.0).clamp_min(1e-12)
    wp = _zero_padded(rows / ws[:, None], plan.n_elems, (plan.cout_pad, plan.k_pad))
    return wp.to(FP8).contiguous(), torch.nn.functional.pad(ws * act_scale, (0, plan.cout_pad - cout), value=1.0)


def _rows_image_split(weight: torch.Tensor, plan: ConvPackPlan):
    """DY_WLAYOUT_ROWS in split float16: (image, inverse row scales).  K order (r, q, c), every 8 channels as [hi x 8 | lo x 8]:
    4 bytes per element, carried as float16 pairs."""
    cout, cin_g, k, _ = weight.shape
    w = weight.to(torch.float32).permute(0, 2, 3, 1).reshape(cout, k * k, cin_g)
    hi, lo, inv = _split_f16x2(torch.nn.functional.pad(w, (0, plan.cin - cin_g)))
    pair = torch.stack((hi.reshape(cout, k * k, plan.cin // 8, 8), lo.reshape(cout, k * k, plan.cin // 8, 8)), 3)  # (cout, taps, groups, 2, 8)
    wp = _zero_padded(pair.reshape(cout, -1), 2 * plan.n_elems, (plan.cout_pad, plan.k_pad * 2))
    return wp, torch.nn.functional.pad(inv, (0, plan.cout_pad - cout), value=1.0)


def _halo3x3_image(weight: torch.Tensor, p: ConvPackPlan, dtype: torch.dtype) -> torch.Tensor:
    """DY_WLAYOUT_HALO3X3 (include/dyolo.h): MFMA-fragment order per (cout tile, K chunk, tap)."""
    wpad = _zero_padded(weight.to(torch.float32), p.n_elems, (p.nt * p.bn, p.nch * p.kc, 3, 3))
    return _permute_cast(wpad.reshape(p.nt, p.bn // 16, 16, p.nch, 4, p.e, 3, 3).permute(0, 3, 6, 7, 1, 4, 2, 5), dtype, p.n_elems)


def _frag1x1_image(w2d: torch.Tensor, p: ConvPackPlan, dtype: torch.dtype) -> torch.Tensor:
    """DY_WLAYOUT_FRAG1X1 (include/dyolo.h) of fp32 (cout, cin) weights: MFMA-fragment order per (cout tile, K group)."""
    wpad = _zero_padded(w2d, p.n_elems, (p.nt * p.bn, p.nch * p.kc))
    return wpad.view(p.nt, p.bn // 16, 16, p.nch, 4, p.e).permute(0, 3, 1, 4, 2, 5).contiguous().view(-1).to(dtype).contiguous()


def _device_pack(src: torch.Tensor, transpose_flip: bool, cin_logical: int, plan: ConvPackPlan, dtype: torch.dtype) -> torch.Tensor:
    """fp32 weights on the GPU -> the packed image in ONE ``dy_pack_conv_weights`` launch (layout + zero padding + cast, transpose + flip
    for the input-gradient convolution), or this step's ``dy_pack_conv_weights_batched`` result when a ``PackCache`` is active."""
    st = src.stride()
    job = (src.data_ptr(), st[0], st[1], st[2], st[3], src.shape[0], src.shape[1], src.shape[2], int(transpose_flip), cin_logical, plan.layout, plan.n_elems)
    cache = _PACK_CACHE["active"]
    if cache is not None and cache.dtype == dtype and cache.lo <= job[0] < cache.hi:
        hit = cache.lookup(job)
        if hit is not None:  # packed by this step's dy_pack_conv_weights_batched launch
            return hit
        out = cache.slot(job, src)
    else:
        out = torch.empty(plan.n_elems, dtype=dtype, device=src.device)
    _launch(lib().dy_pack_conv_weights, job[:10] + (out.data_ptr(), plan.n_elems, dy_dtype(dtype), plan.layout), record=False)
    return out


class PackedConv:
    """Folded + packed weights of one convolution in the layout ``dy_conv2d_nhwc`` expects.

    ``weight``: (cout, cin/groups, k, k) fp32 with BatchNorm / RepVGG branches already folded,
    ``bias``: (cout,) fp32.  Packing = (cout, k, k, cin) row-major, rows padded to k_pad, rows
    count padded to cout_pad with zeros (include/dyolo.h); ``conv_pack_plan`` says which layers take a fragment layout instead.
    """

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, stride: int, pad: int, groups: int, act: bool,
                 dtype: torch.dtype, device, cin_pad: Optional[int] = None, halo: Optional[bool] = None,
                 for_out_f32: bool = False, transpose_flip: bool = False):
        """``halo`` = False forces the generic row layout (both special layouts off); ``for_out_f32``: the conv
        will be called with out_f32=True (Detect heads), which narrows the shapes the streaming kernel is built for.
        ``transpose_flip``: pack W'[ci][co][r][q] = weight[co][ci][k-1-r][k-1-q] (the input-gradient convolution) — device packing only.
        fp32 weights that already live on the device (training: the master weights, every step) are packed by ONE
        ``dy_pack_conv_weights`` launch instead of the host packers' pad / permute / flip / cast chain."""
        dev_pack = weight.is_cuda and weight.dtype == torch.float32 and dtype not in (FP8, F16X2) and groups == 1 and weight.device == torch.device(device)
        if transpose_flip and not dev_pack:
            raise ValueError("PackedConv(transpose_flip=True) needs fp32 weights on the target device")
        self._src = weight if dev_pack else None
        cout, cin_g, k, k2 = weight.shape
        if transpose_flip:
            cout, cin_g = cin_g, cout
        assert k == k2, "square kernels only"
        padded = cin_pad is not None and cin_pad > weight.shape[1]  # the input view carries zero-padded channels (the image: 3 -> one 16-byte chunk)
        if padded and groups != 1:
            raise ValueError("cin_pad is only meaningful for dense convolutions")
        cin = cin_pad if padded else cin_g * groups
        if dtype == F16X2 and groups == 1:
            cin = -(-cin // 8) * 8
        self.act, self.dtype = _act_code(act), dtype  # act: bool (SiLU or none) or a dy_act code
        plan = conv_pack_plan(cout, cin, k, stride, pad, groups, self.act, dtype, halo, for_out_f32)
        self.cout, self.cin, self.k, self.stride, self.pad, self.groups = cout, plan.cin, k, stride, pad, groups
        self.layout, self.k_pad, self.cout_pad = plan.layout, plan.k_pad, plan.cout_pad
        self.wscale, self.act_scale = None, (fp8_act_scale() if dtype == FP8 else 1.0)
        # what a DY_WLAYOUT_ROWS pack of the same layer is built from (``rows()``: calls the special layout's kernels refuse)
        self._rows_args = None if plan.layout == _lib.DY_WLAYOUT_ROWS else (weight, bias, stride, pad, groups, act, dtype, device, cin_pad, for_out_f32, transpose_flip)
        self._rows_pack = None
        if dev_pack:  # (either way packed where the weights live — the CPU for inference setup, the GPU in training: no host round trip)
            self.w = _device_pack(weight.detach(), transpose_flip, cin_pad if padded else 0, plan, dtype)
        else:
            w = weight.detach()
            if padded:
                w = torch.nn.functional.pad(w.float(), (0, 0, 0, 0, 0, cin_pad - cin_g))
            if dtype == F16X2 and groups == 1:
                w, self.wscale = _rows_image_split(w, plan)
            elif dtype == FP8:
                w, self.wscale = _rows_image_fp8(w, plan, self.act_scale)
            elif plan.layout == _lib.DY_WLAYOUT_HALO3X3:
                w = _halo3x3_image(w, plan, dtype)
            elif plan.layout == _lib.DY_WLAYOUT_FRAG1X1:
                w = _frag1x1_image(w.to(torch.float32).reshape(cout, plan.cin), plan, dtype)
            else:  # (grouped split float16: the small-group kernel multiplies joined fp32 inputs by fp32 weights)
                w = _rows_image(w, plan, torch.float32 if dtype == F16X2 else dtype)
            self.w = w.to(device)
            if self.wscale is not None:
                self.wscale = self.wscale.to(device)
        self.b = _padded_bias(bias, plan.cout_pad, weight.device).to(device)

    def rows(self) -> "PackedConv":
        """The same layer packed in DY_WLAYOUT_ROWS (built on first use, kept): the layout every call shape has a kernel for.
        ``conv2d`` takes it when a call does not meet the preconditions of the kernels behind this pack's special layout."""
        if self.layout == _lib.DY_WLAYOUT_ROWS:
            return self
        if self._rows_pack is None:
            w, b, stride, pad, groups, act, dtype, device, cin_pad, for_out_f32, tf = self._rows_args
            self._rows_pack = PackedConv(w, b, stride, pad, groups, act, dtype, device, cin_pad=cin_pad, halo=False, for_out_f32=for_out_f32, transpose_flip=tf)
        return self._rows_pack

    def for_call(self, x_bytes: int, y_bytes: int, ld_y: int, y_ptr: int, residual: bool, out_f32: bool, gathered: bool) -> "PackedConv":
        """This pack, or its DY_WLAYOUT_ROWS twin when the kernels behind DY_WLAYOUT_HALO3X3 do not take the call: csrc decides
        (``dy_conv3x3_halo_route``, the rule ``dy_conv2d_nhwc`` dispatches by)."""
        if self.layout != _lib.DY_WLAYOUT_HALO3X3:
            return self
        route = lib().dy_conv3x3_halo_route(self.cin, self.cout, self.stride, dy_dtype(self.dtype), x_bytes, y_bytes, ld_y, y_ptr, residual, out_f32, gathered)
        return self.rows() if route == _lib.DY_ROUTE_ROWS else self


def conv_out_hw(h: int, w: int, k: int, s: int, p: int) -> Tuple[int, int]:
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def last_kernel_name() -> str:
    """Device kernel the calling thread's last libdyolo launch dispatched to (``dy_last_kernel_name``)."""
    return (lib().dy_last_kernel_name() or b"").decode()


class BnBehind:
    """The train-mode BatchNorm + activation of the layer IN FRONT of a convolution, for that convolution's input gradient
    (``conv_dgrad(bn_behind=)``, ``dy_conv_desc.bnb_z``): when the gradient kernel has the epilogue, the sums that BatchNorm's
    backward needs (du, du * xhat per channel) are in ``state``'s workspace afterwards and ``slots`` says how many partial slots —
    hand it to ``bn_train_bwd(partial_slabs=)``; 0: nothing was written, the backward runs its own reduction.  Only valid when the
    gradient that convolution computes is the WHOLE gradient of that layer's output (no other consumer)."""

    def __init__(self, z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, state: "BnState", act: bool):
        self.z, self.gamma, self.beta, self.state, self.act = z, gamma, beta, state, act
        self.slots = 0


def conv_stats_written() -> int:
    """Partial-sum slots this thread's last ``dy_conv2d_nhwc`` left in ``bn_stats`` (0: the launched kernel has no statistics epilogue)."""
    return int(lib().dy_conv_stats_written())


def conv2d(x: torch.Tensor, pc: PackedConv, out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           out_f32: bool = False, up2x: bool = False, x2: Optional[torch.Tensor] = None, dil2: bool = False,
           bn_stats: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None, bn_behind: Optional[BnBehind] = None) -> torch.Tensor:
    """act(conv(x) + bias) (+ residual) through ``dy_conv2d_nhwc``.

    ``x2``: optional second input whose channels follow x's (Concat folded into the gather);
    ``up2x``: x is consumed through a fused 2x nearest upsample.
    ``dil2``: x is consumed zero-dilated by 2 (value at even (h, w) only): the gather of a stride-2 transposed conv.
    ``bn_stats``: the ``BnState`` of the train-mode BatchNorm that follows: a kernel with the statistics epilogue leaves the output's
    per-channel partial sums in its workspace (``conv_stats_written()`` = how many slots; hand that to ``bn_train_fwd(partial_slabs=)``).
    ``out_dtype``: storage type of the output when it differs from the input's (mixed-precision plans of BASELINE config 5: fp8 ->
    float16 behind an fp8 trunk, float16 -> fp8 into one; ``dy_conv_desc.y_dtype1``, the flat-K kernel).
    """
    require_device(x, "conv2d input")
    if x.dtype != pc.dtype:
        raise TypeError(f"conv2d: input dtype {x.dtype} != packed weight dtype {pc.dtype}")
    n, c1, hb, wb = x.shape
    h, w = (2 * hb, 2 * wb) if (up2x or dil2) else (hb, wb)
    cin = c1 + (x2.shape[1] if x2 is not None else 0)
    if cin != pc.cin:
        raise ValueError(f"conv2d: input has {cin} channels, weights expect {pc.cin}")
    ho, wo = conv_out_hw(h, w, pc.k, pc.stride, pc.pad)
    if out_dtype is not None and out_f32:
        raise ValueError("conv2d: out_dtype and out_f32 exclude each other")
    odt = torch.float32 if out_f32 else (out_dtype or x.dtype)
    if out is None:
        epc_o = chan_gran(odt)  # keep every pixel row 16-byte aligned (vector stores in all kernels)
        out = alloc_nhwc(n, pc.cout, ho, wo, odt, x.device, ld=-(-pc.cout // epc_o) * epc_o)
    elif tuple(out.shape) != (n, pc.cout, ho, wo) or out.dtype != odt:
        raise ValueError(f"conv2d: out has shape {tuple(out.shape)}/{out.dtype}, expected {(n, pc.cout, ho, wo)}/{odt}")
    xp, ldx = view_params(x)
    yp, ldy = view_params(out)
    if odt != x.dtype and not out_f32:
        pc = pc.rows()  # another storage type on the output is built in the flat-K kernel only (DY_WLAYOUT_ROWS)
    pc = pc.for_call(n * hb * wb * ldx * x.element_size(), n * ho * wo * ldy * out.element_size(), ldy, yp, residual is not None, out_f32,
                     x2 is not None or up2x or dil2)
    d = ConvDesc()
    d.x, d.w, d.bias, d.y = xp, pc.w.data_ptr(), pc.b.data_ptr(), yp
    d.batch, d.h, d.w_in, d.cin, d.ld_x = n, h, w, cin, ldx
    d.ho, d.wo, d.cout, d.ld_y = ho, wo, pc.cout, ldy
    d.ksize, d.stride, d.pad, d.groups = pc.k, pc.stride, pc.pad, pc.groups
    d.act, d.dtype, d.out_f32 = pc.act, dy_dtype(x.dtype), int(out_f32)
    d.k_pad, d.cout_pad, d.up2x, d.w_layout = pc.k_pad, pc.cout_pad, (2 if dil2 else int(up2x)), pc.layout
    if bn_stats is not None:
        if bn_stats.c != pc.cout:
            raise ValueError("conv2d: bn_stats must be the BnState of a BatchNorm over the output channels")
        d.bn_stats = bn_stats.ws.data_ptr()
    if bn_behind is not None:
        bb = bn_behind
        if bn_stats is not None or residual is not None or out_f32 or tuple(bb.z.shape) != tuple(out.shape) or bb.z.dtype != x.dtype or bb.state.c != pc.cout:
            raise ValueError("conv2d: bn_behind needs the saved z of the layer in front (shape / dtype of the output) and excludes bn_stats / residual / out_f32")
        if bb.gamma.dtype != torch.float32 or bb.beta.dtype != torch.float32 or not bb.gamma.is_contiguous() or not bb.beta.is_contiguous():
            raise ValueError("conv2d: bn_behind.gamma / beta must be contiguous fp32")
        d.bn_stats = bb.state.ws.data_ptr()
        d.bnb_z, d.bnb_ld_z = view_params(bb.z)
        d.bnb_act = DY_ACT_SILU if bb.act else DY_ACT_NONE
        d.bnb_mean, d.bnb_rstd, d.bnb_gamma, d.bnb_beta = bb.state.mean.data_ptr(), bb.state.rstd.data_ptr(), bb.gamma.data_ptr(), bb.beta.data_ptr()
    if residual is not None:
        if tuple(residual.shape) != tuple(out.shape) or residual.dtype != x.dtype:
            raise ValueError("conv2d: residual must match the output shape and the input dtype")
        d.residual, d.ld_res = view_params(residual)
    if x2 is not None:
        if tuple(x2.shape[2:]) != (h, w) or x2.shape[0] != n or x2.dtype != x.dtype:
            raise ValueError("conv2d: x2 must have the (upsampled) spatial size and dtype of x")
        d.x2, d.ld_x2 = view_params(x2)
        d.cin_split = c1
    if pc.wscale is not None:
        d.w_scale, d.act_scale = pc.wscale.data_ptr(), pc.act_scale
    if odt != x.dtype and not out_f32:
        d.y_dtype1 = dy_dtype(odt) + 1
        if odt == FP8:
            d.act_scale = fp8_act_scale()  # the output quantum (the input is 16-bit: no pack-time scale)
    _launch(lib().dy_conv2d_nhwc, (C.byref(d),), keep=(d, x, out, residual, x2, pc, bn_behind))
    if bn_behind is not None:
        bn_behind.slots = conv_stats_written()
    if _absmax_log is not None and not out_f32:  # activations that WOULD be stored in fp8 (the fp32 head logits are not)
        _absmax_log.append(out.float().abs().amax())
    return out


def quantize_fp8(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """16-bit / fp32 NHWC view -> fp8 (e4m3fn) with the network's activation scale, through ``dy_quantize_fp8_nhwc``."""
    require_device(x, "quantize input")
    n, c, h, w = x.shape
    if c % 16:
        raise ValueError("quantize_fp8: channels must be a multiple of 16 (one fp8 chunk)")
    if out is None:
        out = alloc_nhwc(n, c, h, w, FP8, x.device)
    (xp, ldx), (op, ldo) = view_params(x), view_params(out)
    _launch(lib().dy_quantize_fp8_nhwc, (xp, op, n * h * w, c, ldx, ldo, dy_dtype(x.dtype), fp8_act_scale()), keep=(x, out))
    return out


# ---- fused stem ---------------------------------------------------------------------------------------


class PackedStem:
    """Weights of the first layer Conv(cin<=3, cout, 3, 2) for ``dy_stem_conv3x3s2_nchw``: rows of the folded
    OIHW taps (k = c*9 + r*3 + q) zero padded to 32, rows padded to a multiple of 16 (include/dyolo.h)."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, act: bool, dtype: torch.dtype, device):
        cout, cin, k, k2 = weight.shape
        if not (k == k2 == 3 and cin * 9 <= 32 and cout <= 80):
            raise ValueError("PackedStem: needs a 3x3 kernel, cin <= 3 and cout <= 80")
        self.cout, self.cin, self.dtype = cout, cin, dtype
        self.act = _act_code(act)
        cp = -(-cout // 16) * 16
        wp = _zero_padded(weight.detach().to(torch.float32).cpu().reshape(cout, cin * 9), cp * 32, (cp, 32))
        self.b = _padded_bias(bias.detach().cpu(), cp, "cpu").to(device)
        if dtype == F16X2:  # [hi rows | lo rows | inverse row scales] in one buffer (include/dyolo.h)
            if cout % 8 or cout > 64:
                raise ValueError("PackedStem: split-float16 storage needs cout a multiple of 8 up to 64")
            hi, lo, inv = _split_f16x2(wp)
            raw = torch.cat((hi.reshape(-1).view(torch.uint8), lo.reshape(-1).view(torch.uint8), inv.view(torch.uint8)))
            self.w = raw.contiguous().to(device)
            return
        self.w = wp.to(dtype).contiguous().to(device)


def stem_conv(src: torch.Tensor, ps: PackedStem, out: Optional[torch.Tensor] = None, mark_input: bool = False) -> torch.Tensor:
    """fp32 NCHW image -> act(conv3x3 s2 p1 + bias) as an NHWC view of ``ps.dtype`` (layout cast fused in)."""
    require_device(src, "input")
    if src.dtype != torch.float32 or not src.is_contiguous() or src.dim() != 4 or src.shape[1] != ps.cin:
        raise ValueError(f"stem_conv expects a contiguous fp32 (N,{ps.cin},H,W) tensor")
    n, c, h, w = src.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if out is None:
        e = chan_gran(ps.dtype)
        out = alloc_nhwc(n, ps.cout, ho, wo, ps.dtype, src.device, ld=-(-ps.cout // e) * e)
    op, ld = view_params(out)
    args = (src.data_ptr(), ps.w.data_ptr(), ps.b.data_ptr(), op, n, c, h, w, ps.cout, ld, ps.act, dy_dtype(ps.dtype))
    _launch(lib().dy_stem_conv3x3s2_nchw, args, keep=(out, ps))
    if mark_input and _recording is not None:
        _recording.input_slot = (len(_recording.ops) - 1, 0)
    return out



_STEM_TRAIN_W: dict = {}


def stem_conv_u8(img: torch.Tensor, weight: torch.Tensor, dtype: torch.dtype, divisor: float = 255.0) -> torch.Tensor:
    """Training stem: uint8 NCHW image -> conv3x3 s2 p1 (no bias, no activation) as an NHWC view of ``dtype`` through
    ``dy_stem_conv3x3s2_nchw_u8``.  ``weight``: the fp32 master weight (cout, cin <= 3, 3, 3) on the device — its OIHW rows ARE the
    kernel's k order, so packing is one casting copy into a persistent zero-padded [cout][32] buffer."""
    require_device(img, "training image")
    cout, cin = weight.shape[0], weight.shape[1]
    if img.dtype != torch.uint8 or not img.is_contiguous() or img.shape[1] != cin or tuple(weight.shape[2:]) != (3, 3) or cout % 16 or cout > 80:
        raise ValueError("stem_conv_u8: contiguous uint8 (N, cin, H, W) image, (cout % 16 == 0, cin, 3, 3) weights")
    key = (weight.data_ptr(), cout, cin, dtype, str(img.device))  # (an address may be handed to another model's stem of another width later)
    ent = _STEM_TRAIN_W.get(key)
    if ent is None:
        ent = _STEM_TRAIN_W[key] = (torch.zeros((cout, 32), dtype=dtype, device=img.device), zero_bias(cout, img.device))
    wp, bp = ent
    wp[:, : cin * 9].copy_(weight.detach().reshape(cout, cin * 9))
    n, _, h, w = img.shape
    out = alloc_nhwc(n, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1, dtype, img.device)
    op, ld = view_params(out)
    _launch(lib().dy_stem_conv3x3s2_nchw_u8, (img.data_ptr(), float(divisor), wp.data_ptr(), bp.data_ptr(), op, n, cin, h, w, cout, ld, DY_ACT_NONE, dy_dtype(dtype)),
            keep=(img, wp, bp, out))
    return out


class PackedStem2:
    """Weights of layers 0 + 1 for ``dy_stem2_fused``: the stem rows as in :class:`PackedStem` and the stride-2 3x3
    layer as [64][288] rows with k = (r*3 + q)*32 + c (include/dyolo.h)."""

    def __init__(self, w0, b0, act0: bool, w1, b1, act1: bool, dtype: torch.dtype, device):
        if tuple(w0.shape) != (32, 3, 3, 3) or tuple(w1.shape) != (64, 32, 3, 3):
            raise ValueError("PackedStem2: built for Conv(3, 32, 3, 2) followed by a 3x3 stride-2 32 -> 64 layer")
        self.stem = PackedStem(w0, b0, act0, dtype, device)
        self.dtype = dtype
        self.act1 = _act_code(act1)
        self.w1_scale = None
        if dtype == F16X2:  # layer 1 as dy_conv2d_nhwc's split rows (K order (r, q, c), 8-channel groups [hi x 8 | lo x 8]) + inverse row scales
            self._pc1 = PackedConv(w1.detach().cpu(), b1.detach().cpu(), 2, 1, 1, act1, dtype, device)
            if self._pc1.cout_pad != 64 or self._pc1.k_pad != 288:
                raise ValueError("PackedStem2: unexpected split pack geometry")
            self.w1, self.b1, self.w1_scale = self._pc1.w, self._pc1.b, self._pc1.wscale
            return
        self.w1 = w1.detach().to(torch.float32).cpu().permute(0, 2, 3, 1).reshape(64, 288).to(dtype).contiguous().to(device)
        self.b1 = b1.detach().to(torch.float32).cpu().contiguous().to(device)


def stem2_fused_supported(cin: int, c0: int, c1: int, h: int, w: int, dtype: torch.dtype) -> bool:
    return dtype != FP8 and bool(lib().dy_stem2_fused_supported(cin, c0, c1, h, w, dy_dtype(dtype)))


def stem2_fused(src: torch.Tensor, ps: PackedStem2, out: Optional[torch.Tensor] = None, mark_input: bool = False) -> torch.Tensor:
    """fp32 NCHW image -> layers 0 and 1 (two stride-2 3x3 convolutions with SiLU) as an NHWC view at 1/4 resolution."""
    require_device(src, "input")
    if src.dtype != torch.float32 or not src.is_contiguous() or src.dim() != 4 or src.shape[1] != 3:
        raise ValueError("stem2_fused expects a contiguous fp32 (N,3,H,W) tensor")
    n, _, h, w = src.shape
    if out is None:
        out = alloc_nhwc(n, 64, h // 4, w // 4, ps.dtype, src.device)
    op, ld = view_params(out)
    d = Stem2Desc(x=src.data_ptr(), w0=ps.stem.w.data_ptr(), b0=ps.stem.b.data_ptr(), w1=ps.w1.data_ptr(), b1=ps.b1.data_ptr(), y=op,
                  n=n, h=h, w=w, ld_y=ld, act0=ps.stem.act, act1=ps.act1, dtype=dy_dtype(ps.dtype),
                  w1_scale=ps.w1_scale.data_ptr() if ps.w1_scale is not None else None)
    _launch(lib().dy_stem2_fused, (C.byref(d),), keep=(d, out, ps))
    if mark_input and _recording is not None:
        _recording.input_slot = (len(_recording.ops) - 1, -1)
    return out

# ---- layout ops -------------------------------------------------------------------------------------


def to_nhwc(src: torch.Tensor, dtype: torch.dtype, c_pad: Optional[int] = None, out: Optional[torch.Tensor] = None,
            mark_input: bool = False) -> torch.Tensor:
    """fp32 NCHW (contiguous) -> NHWC view of ``dtype`` with channels zero-padded to ``c_pad``."""
    require_device(src, "input")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("to_nhwc expects a contiguous fp32 NCHW tensor")
    n, c, h, w = src.shape
    epc = chan_gran(dtype)
    c_pad = c_pad or (c + epc - 1) // epc * epc
    if out is None:
        out = alloc_nhwc(n, c_pad, h, w, dtype, src.device)
    op, ld = view_params(out)
    args = (src.data_ptr(), op, n, c, h, w, c_pad, ld, dy_dtype(dtype))
    _launch(lib().dy_nchw_f32_to_nhwc, args, keep=(out,))
    if mark_input and _recording is not None:
        _recording.input_slot = (len(_recording.ops) - 1, 0)
    return out


def u8_to_nhwc(src: torch.Tensor, dtype: torch.dtype, divisor: float = 255.0) -> torch.Tensor:
    """uint8 NCHW (contiguous) -> NHWC view of ``dtype`` holding src / divisor, channels zero-padded to one chunk."""
    require_device(src, "input")
    if src.dtype != torch.uint8 or not src.is_contiguous() or src.dim() != 4:
        raise ValueError("u8_to_nhwc expects a contiguous uint8 NCHW tensor")
    n, c, h, w = src.shape
    epc = elems_per_chunk(dtype)
    c_pad = (c + epc - 1) // epc * epc
    out = alloc_nhwc(n, c_pad, h, w, dtype, src.device)
    op, ld = view_params(out)
    _launch(lib().dy_nchw_u8_to_nhwc, (src.data_ptr(), op, n, c, h, w, c_pad, ld, divisor, dy_dtype(dtype)), keep=(src, out))
    return out


def to_nchw_f32(x: torch.Tensor) -> torch.Tensor:
    """NHWC view -> contiguous fp32 NCHW tensor (module-level parity checks, user hand-back)."""
    require_device(x)
    n, c, h, w = x.shape
    xp, ld = view_params(x)
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    _launch(lib().dy_nhwc_to_nchw_f32, (xp, out.data_ptr(), n, c, h, w, ld, dy_dtype(x.dtype)), keep=(x, out))
    return out


def upsample2x(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    require_device(x)
    n, c, h, w = x.shape
    if out is None:
        out = alloc_nhwc(n, c, 2 * h, 2 * w, x.dtype, x.device)
    xp, lds = view_params(x)
    op, ldd = view_params(out)
    _launch(lib().dy_upsample2x_nhwc, (xp, op, n, h, w, c, lds, ldd, dy_dtype(x.dtype)), keep=(x, out))
    return out


def copy_nhwc(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    require_device(x)
    n, c, h, w = x.shape
    xp, lds = view_params(x)
    op, ldd = view_params(out)
    _launch(lib().dy_copy_nhwc, (xp, op, n, h, w, c, lds, ldd, dy_dtype(x.dtype)), keep=(x, out))
    return out


def sppf_maxpool3(x: torch.Tensor, y1: torch.Tensor, y2: torch.Tensor, y3: torch.Tensor, k: int) -> None:
    require_device(x)
    n, c, h, w = x.shape
    xp, ld = view_params(x)
    ptrs = []
    for y in (y1, y2, y3):
        p, l2 = view_params(y)
        if l2 != ld or tuple(y.shape) != tuple(x.shape):
            raise ValueError("sppf_maxpool3: outputs must be slices of the same buffer as x")
        ptrs.append(p)
    _launch(lib().dy_sppf_maxpool3, (xp, *ptrs, n, h, w, c, ld, k, dy_dtype(x.dtype)), keep=(x, y1, y2, y3))


# ---- detect decode + NMS --------------------------------------------------------------------------


def _attach_filter(d, who: str, nms_bufs: "NmsBuffers", n: int, anchors: int, conf_thres: float, classes_mask: Optional[torch.Tensor]) -> None:
    """Point a decode descriptor's fused NMS candidate filter at ``nms_bufs.workspace`` (then ``nms(..., prefiltered=True)`` with the
    same buffers, conf_thres and classes_mask)."""
    if (nms_bufs.batch, nms_bufs.anchors) != (n, anchors):
        raise ValueError(f"{who}: nms_bufs were sized for another batch / anchor count")
    d.nms_workspace, d.nms_workspace_bytes = nms_bufs.workspace.data_ptr(), nms_bufs.workspace.numel()
    d.conf_thres = conf_thres
    d.classes_mask = classes_mask.data_ptr() if classes_mask is not None else None


def detect_decode(levels: Sequence[torch.Tensor], strides: Sequence[float], nc: int, reg_max: int,
                  out: Optional[torch.Tensor] = None, nms_bufs: Optional["NmsBuffers"] = None, conf_thres: float = 0.25,
                  classes_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """levels[i]: fp32 NHWC view (N, 4*reg_max+nc, H_i, W_i) -> (N, 4+nc, A) fp32.

    ``nms_bufs``: fuse the NMS candidate filter into this pass (then call ``nms(..., prefiltered=True)``
    with the same buffers, conf_thres and classes_mask)."""
    n = levels[0].shape[0]
    d = DecodeDesc()
    A = 0
    for i, t in enumerate(levels):
        require_device(t)
        if t.dtype != torch.float32 or t.shape[1] != 4 * reg_max + nc:
            raise ValueError("detect_decode: levels must be fp32 with 4*reg_max+nc channels")
        p, ld = view_params(t)
        d.level[i], d.h[i], d.w[i], d.ld[i], d.stride[i] = p, t.shape[2], t.shape[3], ld, float(strides[i])
        A += t.shape[2] * t.shape[3]
    d.n_levels, d.batch, d.nc, d.reg_max = len(levels), n, nc, reg_max
    if out is None:
        out = torch.empty((n, 4 + nc, A), dtype=torch.float32, device=levels[0].device)
    d.out = out.data_ptr()
    if nms_bufs is not None:
        _attach_filter(d, "detect_decode", nms_bufs, n, A, conf_thres, classes_mask)
    _launch(lib().dy_detect_decode, (C.byref(d),), keep=(d, out, nms_bufs, classes_mask, *levels))
    return out


def branch_fused_supported(c_in: int, c_mid: int, c_out: int, kind: int, nc: int, reg_max: int, dtype: torch.dtype) -> bool:
    return dtype in (torch.bfloat16, torch.float16) and bool(lib().dy_detect_branch_fused_supported(c_in, c_mid, c_out, kind, nc, reg_max, dy_dtype(dtype)))


def nms_reset_counts(bufs: "NmsBuffers") -> None:
    """Zero the per-image candidate counts: once per pass, before the first class branch appends candidates."""
    _launch(lib().dy_nms_reset_counts, (bufs.workspace.data_ptr(), bufs.batch), keep=(bufs,))


def detect_branch_fused(x: torch.Tensor, pc3: "PackedConv", w1: torch.Tensor, b1: torch.Tensor, kind: int, nc: int, reg_max: int, stride: float, pred: torch.Tensor,
                        anchor0: int, nms_bufs: Optional["NmsBuffers"] = None, conf_thres: float = 0.25, classes_mask: Optional[torch.Tensor] = None) -> None:
    """One Detect branch (kind 1 = box, 2 = class) of one level from its second 3x3 conv to rows of ``pred`` through
    ``dy_detect_branch_fused``.  x: the branch's first conv output (N, 64, H, W); pc3: the 3x3 Conv packed in
    DY_WLAYOUT_HALO3X3; (w1, b1): ``pack_frag1x1`` of the plain 1x1 conv."""
    require_device(x, "branch input")
    if pc3.layout != _lib.DY_WLAYOUT_HALO3X3 or pc3.dtype != x.dtype or pc3.k != 3 or pc3.stride != 1:
        raise ValueError("detect_branch_fused: the 3x3 conv must be packed in DY_WLAYOUT_HALO3X3 for x's dtype")
    n, c, h, w = x.shape
    d = BranchDesc()
    d.x, d.ld_x = view_params(x)
    d.w3, d.b3, d.w1, d.b1, d.out = pc3.w.data_ptr(), pc3.b.data_ptr(), w1.data_ptr(), b1.data_ptr(), pred.data_ptr()
    d.batch, d.h, d.w, d.c_in, d.c_mid, d.nc, d.reg_max, d.kind, d.dtype = n, h, w, c, pc3.cout, nc, reg_max, kind, dy_dtype(x.dtype)
    d.anchors, d.anchor0, d.stride = pred.shape[2], anchor0, float(stride)
    if pc3.act not in (DY_ACT_SILU, DY_ACT_SILU_L2E):
        raise ValueError("detect_branch_fused: the 3x3 conv must end in SiLU")
    d.act_l2e = int(pc3.act == DY_ACT_SILU_L2E)  # (the caller packed w1 divided by log2 e then: the logits stay in true units)
    if pred.dtype != torch.float32 or pred.shape[0] != n or pred.shape[1] != 4 + nc or not pred.is_contiguous():
        raise ValueError("detect_branch_fused: pred must be a contiguous fp32 (N, 4 + nc, A) tensor")
    if kind == 2 and nms_bufs is not None:
        _attach_filter(d, "detect_branch_fused", nms_bufs, n, pred.shape[2], conf_thres, classes_mask)
    _launch(lib().dy_detect_branch_fused, (C.byref(d),), keep=(d, x, pc3, w1, b1, pred, nms_bufs, classes_mask))


def pack_frag1x1(weight: torch.Tensor, bias: torch.Tensor, dtype: torch.dtype, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(cout, cin[,1,1]) weights + bias in DY_WLAYOUT_FRAG1X1 order (include/dyolo.h), whatever kernel PackedConv would pick."""
    w2 = weight.detach().to(torch.float32).cpu().reshape(weight.shape[0], -1)
    dt = torch.float16 if dtype == F16X2 else dtype
    plan = _frag1x1_plan(*w2.shape, dt)
    bp = _padded_bias(bias.detach().cpu(), plan.cout_pad, "cpu")
    if dtype != F16X2:
        return _frag1x1_image(w2, plan, dt).to(device), bp.to(device)
    # split float16 (dy_detect_head_decode with DY_F16X2): the float16 fragment image of the hi halves, then of the lo halves; bias
    # followed by the inverse row scales
    hi, lo, inv = _split_f16x2(w2)
    wp = torch.cat([_frag1x1_image(h.to(torch.float32), plan, dt) for h in (hi, lo)])
    return wp.to(device), torch.cat((bp, torch.nn.functional.pad(inv, (0, plan.cout_pad - inv.numel()), value=1.0))).to(device)


def head_decode_supported(c_box: int, c_cls: int, nc: int, reg_max: int, dtype: torch.dtype) -> bool:
    return dtype != FP8 and bool(lib().dy_detect_head_decode_supported(c_box, c_cls, nc, reg_max, dy_dtype(dtype)))


def detect_head_decode(x_box: Sequence[torch.Tensor], x_cls: Sequence[torch.Tensor], packed_box, packed_cls,
                       strides: Sequence[float], nc: int, reg_max: int, out: Optional[torch.Tensor] = None,
                       nms_bufs: Optional["NmsBuffers"] = None, conf_thres: float = 0.25,
                       classes_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Last 1x1 convs of both Detect branches + decode (+ NMS candidate filter) in one ``dy_detect_head_decode`` pass.

    x_box[i] / x_cls[i]: NHWC views (N, c, H_i, W_i), the inputs of cv2[i][2] / cv3[i][2]; packed_box[i] / packed_cls[i]:
    ``pack_frag1x1`` (w, b) of those convs.  Returns (N, 4+nc, A) fp32."""
    n = x_box[0].shape[0]
    d = HeadDecodeDesc()
    A = 0
    for i, (tb, tc) in enumerate(zip(x_box, x_cls)):
        require_device(tb)
        require_device(tc)
        if tb.dtype != tc.dtype or tb.shape[2:] != tc.shape[2:] or tb.shape[0] != n or tc.shape[0] != n:
            raise ValueError("detect_head_decode: branch inputs of one level must agree in dtype and size")
        if tb.shape[1] != x_box[0].shape[1] or tc.shape[1] != x_cls[0].shape[1] or tb.dtype != x_box[0].dtype:
            raise ValueError("detect_head_decode: all levels must have the same branch widths and dtype")
        (d.x_box[i], d.ld_box[i]), (d.x_cls[i], d.ld_cls[i]) = view_params(tb), view_params(tc)
        d.w_box[i], d.b_box[i] = packed_box[i][0].data_ptr(), packed_box[i][1].data_ptr()
        d.w_cls[i], d.b_cls[i] = packed_cls[i][0].data_ptr(), packed_cls[i][1].data_ptr()
        d.h[i], d.w[i], d.stride[i] = tb.shape[2], tb.shape[3], float(strides[i])
        A += tb.shape[2] * tb.shape[3]
    d.n_levels, d.batch, d.nc, d.reg_max = len(x_box), n, nc, reg_max
    d.c_box, d.c_cls, d.dtype = x_box[0].shape[1], x_cls[0].shape[1], dy_dtype(x_box[0].dtype)
    if out is None:
        out = torch.empty((n, 4 + nc, A), dtype=torch.float32, device=x_box[0].device)
    d.out = out.data_ptr()
    if nms_bufs is not None:
        _attach_filter(d, "detect_head_decode", nms_bufs, n, A, conf_thres, classes_mask)
    _launch(lib().dy_detect_head_decode, (C.byref(d),),
            keep=(d, out, nms_bufs, classes_mask, *x_box, *x_cls, *packed_box, *packed_cls))
    return out


class NmsBuffers:
    """Persistent outputs + workspace of ``dy_nms`` for one (batch, anchors, max_det)."""

    ROW = 6  # x1, y1, x2, y2, conf, cls

    def __init__(self, batch: int, anchors: int, max_det: int, device, candidates_per_anchor: int = 1):
        """``candidates_per_anchor``: nc for the validator's multi_label NMS (one candidate per (anchor, class) pair), else 1."""
        self.batch, self.anchors, self.max_det, self.cpa = batch, anchors, max_det, candidates_per_anchor
        self.workspace = torch.empty((self.workspace_bytes(),), dtype=torch.uint8, device=device)
        self.out = torch.empty((batch, max_det, self.ROW), dtype=torch.float32, device=device)
        self.count = torch.empty((batch,), dtype=torch.int32, device=device)
        self.index = torch.empty((batch, max_det), dtype=torch.int32, device=device)

    def workspace_bytes(self) -> int:
        return lib().dy_nms_workspace_bytes(self.batch, self.anchors * self.cpa)


def _nms_desc(pred: torch.Tensor, bufs: NmsBuffers, nc: int, conf_thres: float, iou_thres: float, max_nms: int, max_wh: float, agnostic: bool,
              classes_mask: Optional[torch.Tensor], prefiltered: bool, multi_label: bool) -> NmsDesc:
    """The ``dy_nms_desc`` of a call on ``pred`` (N, 4 + nc (+ extra), A) into ``bufs``."""
    n, ch, A = pred.shape
    d = NmsDesc()
    d.pred, d.batch, d.nc, d.n_extra, d.anchors = pred.data_ptr(), n, nc, ch - 4 - nc, A
    d.conf_thres, d.iou_thres, d.max_det, d.max_nms = conf_thres, iou_thres, bufs.max_det, max_nms
    d.max_wh, d.agnostic = max_wh, int(agnostic)
    d.classes_mask = classes_mask.data_ptr() if classes_mask is not None else None
    d.out, d.out_count, d.out_index = bufs.out.data_ptr(), bufs.count.data_ptr(), bufs.index.data_ptr()
    d.workspace, d.workspace_bytes = bufs.workspace.data_ptr(), bufs.workspace.numel()
    d.prefiltered, d.multi_label = int(prefiltered), int(bool(multi_label))
    return d


def nms(pred: torch.Tensor, conf_thres: float, iou_thres: float, max_det: int = 300, max_nms: int = 30000,
        max_wh: float = 7680.0, agnostic: bool = False, nc: int = 0, classes_mask: Optional[torch.Tensor] = None,
        bufs: Optional[NmsBuffers] = None, prefiltered: bool = False, multi_label: bool = False) -> NmsBuffers:
    """Batched NMS on (N, 4+nc(+nm), A) fp32 predictions; results stay on the device.
    ``prefiltered``: ``bufs.workspace`` already holds the candidates (detect_decode(nms_bufs=bufs)).
    ``multi_label``: the validator's form (utils/ops.py:286-288): every (anchor, class) pair above conf is a candidate."""
    require_device(pred, "prediction")
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() != 3:
        raise ValueError("nms expects a contiguous fp32 (N, 4+nc, A) tensor")
    n, ch, A = pred.shape
    nc = nc or ch - 4
    cpa = nc if (multi_label and nc > 1) else 1
    if bufs is None or (bufs.batch, bufs.anchors, bufs.max_det) != (n, A, max_det) or getattr(bufs, "cpa", 1) < cpa:
        if prefiltered:
            raise ValueError("nms(prefiltered=True) needs the NmsBuffers that detect_decode filled")
        bufs = NmsBuffers(n, A, max_det, pred.device, candidates_per_anchor=cpa)
    d = _nms_desc(pred, bufs, nc, conf_thres, iou_thres, max_nms, max_wh, agnostic, classes_mask, prefiltered, multi_label)
    _launch(lib().dy_nms, (C.byref(d),), keep=(d, pred, bufs, classes_mask))
    return bufs


def scale_boxes_(bufs: NmsBuffers, params: torch.Tensor) -> None:
    """In-place scale_boxes + clip_boxes of the kept rows; params: device fp32 (N,5)."""
    _launch(lib().dy_scale_boxes, (bufs.out.data_ptr(), bufs.count.data_ptr(), params.data_ptr(), bufs.batch, bufs.max_det),
            keep=(bufs, params))


# ---- oriented boxes: rotated decode, ProbIoU fast NMS, regularize + scale of the kept rows ---------------------------------------
def obb_decode(levels: Sequence[torch.Tensor], strides: Sequence[float], pred: torch.Tensor, nc: int,
               theta: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dy_obb_decode`` behind the Detect kernels.  ``levels``: the per-level angle logits, fp32 NHWC views (N, 1, h_i, w_i) in true units;
    ``pred``: the decoded (N, 4 + nc(+extra), A) fp32 tensor, whose rows 0 and 1 are turned in place about the anchor points.
    Returns ``theta`` (N, A) fp32 = (sigmoid(logit) - 0.25) * pi."""
    require_device(pred, "prediction")
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() != 3 or pred.shape[1] < 4 + nc:
        raise ValueError("obb_decode expects a contiguous fp32 (N, 4+nc, A) tensor")
    n, ch, A = pred.shape
    if len(levels) > _lib.DY_MAX_LEVELS or len(levels) != len(strides):
        raise ValueError("obb_decode: one stride per level, at most DY_MAX_LEVELS levels")
    if theta is None:
        theta = torch.empty((n, A), dtype=torch.float32, device=pred.device)
    elif tuple(theta.shape) != (n, A) or theta.dtype != torch.float32 or not theta.is_contiguous():
        raise ValueError("obb_decode: theta must be a contiguous fp32 (N, A) tensor")
    d = _lib.ObbDecodeDesc()
    for i, t in enumerate(levels):
        require_device(t, "angle map")
        if t.dtype != torch.float32 or t.shape[0] != n or t.shape[1] < 1:
            raise ValueError("obb_decode: angle maps must be fp32 (N, 1, h, w) NHWC views")
        d.level[i], d.ld[i] = view_params(t)
        d.h[i], d.w[i], d.stride[i] = t.shape[2], t.shape[3], float(strides[i])
    d.n_levels, d.batch, d.nc, d.n_extra, d.anchors = len(levels), n, nc, ch - 4 - nc, A
    d.pred, d.theta = pred.data_ptr(), theta.data_ptr()
    _launch(lib().dy_obb_decode, (C.byref(d),), keep=(d, pred, theta, *levels))
    return theta


class RNmsBuffers(NmsBuffers):
    """Persistent outputs + workspace of ``dy_nms_rotated`` for one (batch, anchors, max_det).  ``out`` (N, max_det, 7) = x, y, w, h, theta,
    conf, cls.  The head of ``workspace`` is a ``dy_nms`` workspace, so the fused Detect candidate filters fill it as they fill
    ``NmsBuffers.workspace``."""

    ROW = 7

    def workspace_bytes(self) -> int:
        """``candidates_per_anchor`` 1: ``dy_nms_rotated``'s size; nc: ``dy_nms_rotated_ml``'s (keys and table for anchors * nc candidates)."""
        if self.cpa == 1:
            return lib().dy_nms_rotated_workspace_bytes(self.batch, self.anchors)
        return lib().dy_nms_rotated_ml_workspace_bytes(self.batch, self.anchors, self.cpa)


def _check_rotated_pred(who: str, pred: torch.Tensor, theta: torch.Tensor) -> Tuple[int, int, int]:
    """The ``pred`` / ``theta`` checks of ``nms_rotated`` and ``nms_rotated_ml``; returns ``pred.shape``."""
    require_device(pred, "prediction")
    require_device(theta, "angles")
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() != 3:
        raise ValueError(f"{who} expects a contiguous fp32 (N, 4+nc, A) tensor")
    n, ch, A = pred.shape
    if tuple(theta.shape) != (n, A) or theta.dtype != torch.float32 or not theta.is_contiguous():
        raise ValueError(f"{who}: theta must be a contiguous fp32 (N, A) tensor")
    return n, ch, A


def nms_rotated(pred: torch.Tensor, theta: torch.Tensor, conf_thres: float, iou_thres: float, max_det: int = 300, max_nms: int = 30000,
                max_wh: float = 7680.0, agnostic: bool = False, nc: int = 0, classes_mask: Optional[torch.Tensor] = None,
                bufs: Optional[RNmsBuffers] = None, prefiltered: bool = False, multi_label: bool = False) -> RNmsBuffers:
    """Batched ProbIoU fast NMS (``dy_nms_rotated``) on (N, 4+nc(+extra), A) fp32 predictions and their (N, A) angles; results stay on the
    device.  ``prefiltered``: ``bufs.workspace`` already holds the candidates (detect_decode(nms_bufs=bufs))."""
    n, ch, A = _check_rotated_pred("nms_rotated", pred, theta)
    nc = nc or ch - 4
    if bufs is None or (bufs.batch, bufs.anchors, bufs.max_det) != (n, A, max_det):
        if prefiltered:
            raise ValueError("nms_rotated(prefiltered=True) needs the RNmsBuffers that detect_decode filled")
        bufs = RNmsBuffers(n, A, max_det, pred.device)
    d = _nms_desc(pred, bufs, nc, conf_thres, iou_thres, max_nms, max_wh, agnostic, classes_mask, prefiltered, multi_label)
    _launch(lib().dy_nms_rotated, (C.byref(d), theta.data_ptr()), keep=(d, pred, theta, bufs, classes_mask))
    return bufs


def nms_rotated_ml(pred: torch.Tensor, theta: torch.Tensor, conf_thres: float, iou_thres: float, max_det: int = 300, max_nms: int = 30000,
                   max_wh: float = 7680.0, agnostic: bool = False, nc: int = 0, classes_mask: Optional[torch.Tensor] = None,
                   bufs: Optional[RNmsBuffers] = None) -> RNmsBuffers:
    """The validator's rotated NMS (``dy_nms_rotated_ml``: ``non_max_suppression(rotated=True, multi_label=True)``): every (anchor, class)
    pair above ``conf_thres`` is a candidate, ``bufs.index`` holds the pair's anchor and column 6 of a row its class.  ``nc`` 1 is the
    single-label form.  Results stay on the device."""
    n, ch, A = _check_rotated_pred("nms_rotated_ml", pred, theta)
    nc = nc or ch - 4
    if bufs is None or (bufs.batch, bufs.anchors, bufs.max_det) != (n, A, max_det) or bufs.cpa != nc:
        bufs = RNmsBuffers(n, A, max_det, pred.device, candidates_per_anchor=nc)
    d = _nms_desc(pred, bufs, nc, conf_thres, iou_thres, max_nms, max_wh, agnostic, classes_mask, False, True)
    _launch(lib().dy_nms_rotated_ml, (C.byref(d), theta.data_ptr()), keep=(d, pred, theta, bufs, classes_mask))
    return bufs


def scale_rboxes_(bufs: RNmsBuffers, params: torch.Tensor) -> None:
    """In-place regularize_rboxes + scale_boxes(xywh=True) + clip_boxes of the kept rows; params: device fp32 (N,5)."""
    _launch(lib().dy_scale_rboxes, (bufs.out.data_ptr(), bufs.count.data_ptr(), params.data_ptr(), bufs.batch, bufs.max_det),
            keep=(bufs, params))


# ---- instance segmentation: Proto's transposed convolution, coefficient gather, mask assembly ------------------------------------
NM = 32  # mask coefficients per detection the kernels are built for (Segment's default nm)


def deconv2x2_as_conv1x1(weight: torch.Tensor, bias: Optional[torch.Tensor]):
    """nn.ConvTranspose2d(cin, cout, 2, 2, 0) weights (cin, cout, 2, 2) -> the (4 * cout, cin, 1, 1) weights and (4 * cout) bias of the 1x1
    convolution whose output ``depth_to_space2`` turns into the transposed convolution's: row (a * 2 + b) * cout + o = W[:, o, a, b]."""
    cin, cout, kh, kw = weight.shape
    if (kh, kw) != (2, 2):
        raise ValueError("deconv2x2_as_conv1x1: a 2 x 2 kernel is expected")
    w = weight.detach().float().permute(2, 3, 1, 0).reshape(4 * cout, cin, 1, 1).contiguous()
    b = torch.zeros(cout, device=weight.device) if bias is None else bias.detach().float()
    return w, b.repeat(4)


def depth_to_space2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n, 4c, h, w) -> (n, c, 2h, 2w), out[:, o, 2y + a, 2x + b] = x[:, (a * 2 + b) * c + o, y, x] (``dy_depth_to_space2_nhwc``)."""
    require_device(x, "depth_to_space2 input")
    n, c4, h, w = x.shape
    if c4 % 4:
        raise ValueError("depth_to_space2: the channel count must be a multiple of 4")
    c = c4 // 4
    if out is None:
        out = alloc_nhwc(n, c, 2 * h, 2 * w, x.dtype, x.device)
    elif tuple(out.shape) != (n, c, 2 * h, 2 * w) or out.dtype != x.dtype:
        raise ValueError(f"depth_to_space2: out has shape {tuple(out.shape)}/{out.dtype}, expected {(n, c, 2 * h, 2 * w)}/{x.dtype}")
    xp, lds = view_params(x)
    op, ldd = view_params(out)
    _launch(lib().dy_depth_to_space2_nhwc, (xp, op, n, h, w, c, lds, ldd, dy_dtype(x.dtype)), keep=(x, out))
    return out


def conv_transpose2x2(x: torch.Tensor, pc: PackedConv, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ConvTranspose2d(k=2, s=2, p=0): ``pc`` = PackedConv of ``deconv2x2_as_conv1x1``'s weights; the 1x1 GEMM, then the depth-to-space."""
    return depth_to_space2(conv2d(x, pc), out=out)


def mask_gather(bufs: NmsBuffers, levels: Optional[Sequence[torch.Tensor]] = None, pred: Optional[torch.Tensor] = None, nc: int = 0,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The kept rows' unscaled boxes and mask coefficients -> (N, max_det, 4 + 32) fp32 (``dy_mask_gather``; call it behind ``nms`` and in
    front of ``scale_boxes_``).  ``levels``: the per-level fp32 NHWC coefficient maps (N, 32, h_i, w_i) of Segment.cv4; or ``pred``: the
    (N, 4 + nc + 32, A) prediction tensor.  Rows beyond the counts are left as they are."""
    d = _lib.MaskGatherDesc()
    n, md = bufs.batch, bufs.max_det
    if out is None:
        out = torch.zeros((n, md, 4 + NM), dtype=torch.float32, device=bufs.out.device)
    elif tuple(out.shape) != (n, md, 4 + NM) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("mask_gather: out must be a contiguous fp32 (N, max_det, 36) tensor")
    d.rows, d.counts, d.index, d.out = bufs.out.data_ptr(), bufs.count.data_ptr(), bufs.index.data_ptr(), out.data_ptr()
    d.batch, d.max_det, d.nm, d.anchors = n, md, NM, bufs.anchors
    keep = [d, bufs, out]
    if (levels is None) == (pred is None):
        raise ValueError("mask_gather: give either the per-level coefficient maps or the prediction tensor")
    if pred is not None:
        require_device(pred, "prediction")
        if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() != 3 or pred.shape[0] != n or pred.shape[2] != bufs.anchors \
                or pred.shape[1] != 4 + nc + NM:
            raise ValueError("mask_gather: pred must be a contiguous fp32 (N, 4 + nc + 32, A) tensor")
        d.pred, d.pred_ch, d.pred_c0 = pred.data_ptr(), pred.shape[1], 4 + nc
        keep.append(pred)
    else:
        if len(levels) > _lib.DY_MAX_LEVELS:
            raise ValueError("mask_gather: too many levels")
        for i, t in enumerate(levels):
            require_device(t, "coefficient map")
            if t.dtype != torch.float32 or t.shape[0] != n or t.shape[1] != NM:
                raise ValueError("mask_gather: coefficient maps must be fp32 (N, 32, h, w) NHWC views")
            d.level[i], d.ld[i] = view_params(t)
            d.h[i], d.w[i] = t.shape[2], t.shape[3]
        d.n_levels = len(levels)
        keep.extend(levels)
    _launch(lib().dy_mask_gather, (C.byref(d),), keep=keep)
    return out


def process_mask(protos: torch.Tensor, side: torch.Tensor, count: torch.Tensor, counts_host: Sequence[int], out_hw: Tuple[int, int],
                 ratio: Tuple[float, float] = (1.0, 1.0), windows: Optional[Sequence[Sequence[int]]] = None,
                 crop_rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The masks of a batch in one ``dy_process_mask`` launch: uint8 (sum(counts), oh, ow), freshly allocated unless ``out`` is given: a
    contiguous uint8 device tensor of sum(counts) * oh * ow elements at an 8-byte aligned address (any shape; it may be a slice of a larger
    buffer), returned viewed as (sum(counts), oh, ow).
    ``protos``: fp32 NHWC view (N, 32, mh, mw); ``side``: ``mask_gather``'s output; ``count``: the device counts and ``counts_host`` their
    values on the host (the predictor reads them back anyway); ``ratio`` = (mw / iw, mh / ih): proto pixels per input-image pixel, for the
    crop at proto resolution (ops.process_mask).  ``crop_rows`` (the rows after ``scale_boxes_``) switches to the retina form
    (ops.process_mask_native): resize ``windows[b]`` = (top, left, sh, sw) of the grid to (oh, ow), crop there."""
    n, nm, mh, mw = protos.shape
    if protos.dtype != torch.float32 or side.dtype != torch.float32 or not side.is_contiguous() or side.shape[0] != n or side.shape[2] != 4 + nm:
        raise ValueError("process_mask: protos must be fp32 (N, nm, mh, mw), side a contiguous fp32 (N, max_det, 4 + nm) tensor")
    md = side.shape[1]
    counts_host = [int(k) for k in counts_host]
    if len(counts_host) != n or any(k < 0 or k > md for k in counts_host):
        raise ValueError("process_mask: counts_host must hold one count in [0, max_det] per image")
    total = sum(counts_host)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if out is not None:  # checked before anything touches the device; the kernel stores 64-bit words into out, so each clause guards memory
        bad = ("its dtype is not uint8" if out.dtype != torch.uint8 else
               f"it holds {out.numel()} elements, not {total} * {oh} * {ow}" if out.numel() != total * oh * ow else
               "it is not contiguous" if not out.is_contiguous() else
               "its address is not 8-byte aligned" if out.data_ptr() % 8 else
               f"it is on '{out.device}', not on the prototypes' device '{protos.device}'" if not out.is_cuda or out.device != protos.device else None)
        if bad:
            raise ValueError(f"process_mask: out must be a contiguous, 8-byte aligned uint8 tensor of sum(counts) * oh * ow elements on the prototypes' device: {bad}")
        out = out.view(total, oh, ow)
    require_device(protos, "protos")
    if out is None:
        out = torch.empty((total, oh, ow), dtype=torch.uint8, device=protos.device)
    d = _lib.ProcessMaskDesc()
    d.protos, d.ld_p = view_params(protos)
    d.batch, d.max_det, d.nm, d.mh, d.mw, d.oh, d.ow, d.total = n, md, nm, mh, mw, oh, ow, total
    d.ratio_x, d.ratio_y = float(ratio[0]), float(ratio[1])
    if nm != NM:
        raise NotImplementedError(f"process_mask: {nm} mask coefficients; dy_process_mask is built for {NM}")
    if total == 0:
        return out
    offs = [0]
    for k in counts_host:
        offs.append(offs[-1] + k)
    win = [list(map(int, w)) for w in windows] if windows is not None else [[0, 0, mh, mw]] * n
    if len(win) != n:
        raise ValueError("process_mask: one window per image")
    table = torch.tensor(offs + [v for w in win for v in w], dtype=torch.int32).to(protos.device, non_blocking=True)
    d.side, d.counts, d.offsets, d.window, d.out = side.data_ptr(), count.data_ptr(), table.data_ptr(), table[n + 1 :].data_ptr(), out.data_ptr()
    if crop_rows is not None:
        if crop_rows.dtype != torch.float32 or tuple(crop_rows.shape) != (n, md, 6) or not crop_rows.is_contiguous():
            raise ValueError("process_mask: crop_rows must be the contiguous fp32 (N, max_det, 6) rows")
        d.crop_rows, d.crop_at_output = crop_rows.data_ptr(), 1
    _launch(lib().dy_process_mask, (C.byref(d),), keep=(d, protos, side, count, table, out, crop_rows))
    return out


def _val_match(fn, bufs: NmsBuffers, tbox: torch.Tensor, tcls: torch.Tensor, timg: torch.Tensor, iouv: Sequence[float],
               clip_wh: Tuple[float, float], single_cls: bool, want_best: bool):
    """The launch behind ``val_match`` / ``val_match_rotated``: ``tbox`` as the kernel reads it (fp32, contiguous, on the device); ``tcls`` /
    ``timg`` are converted here to fp32 / int32."""
    n, max_det, dev = bufs.batch, bufs.max_det, bufs.out.device
    L = int(tbox.shape[0])
    if L:
        tcls = tcls.reshape(-1).to(torch.float32).contiguous()
        timg = timg.reshape(-1).to(torch.int32).contiguous()
    thr = (C.c_float * len(iouv))(*[float(v) for v in iouv])
    tp = torch.empty((n, max_det, len(iouv)), dtype=torch.uint8, device=dev)
    best_iou = torch.empty((n, max_det), dtype=torch.float32, device=dev) if want_best else None
    best_label = torch.empty((n, max_det), dtype=torch.int32, device=dev) if want_best else None
    d = ValMatchDesc()
    d.rows, d.counts = bufs.out.data_ptr(), bufs.count.data_ptr()
    d.tbox, d.tcls, d.timg = (tbox.data_ptr(), tcls.data_ptr(), timg.data_ptr()) if L else (None, None, None)
    d.iouv = thr
    d.batch, d.max_det, d.n_labels, d.n_iouv = n, max_det, L, len(iouv)
    d.clip_w, d.clip_h, d.single_cls = float(clip_wh[0]), float(clip_wh[1]), int(bool(single_cls))
    d.tp = tp.data_ptr()
    d.best_iou = best_iou.data_ptr() if want_best else None
    d.best_label = best_label.data_ptr() if want_best else None
    _launch(fn, (C.byref(d),), keep=(d, thr, bufs, tbox, tcls, timg, tp, best_iou, best_label))
    return (tp, best_iou, best_label) if want_best else tp


def _check_labels(who: str, what: str, cols: int, tbox: torch.Tensor, tcls: torch.Tensor, timg: torch.Tensor) -> int:
    """The label checks of ``val_match`` / ``val_match_rotated``; returns L."""
    L = int(tbox.shape[0])
    if L:
        for t in (tbox, tcls, timg):
            require_device(t, "label")
        if tbox.dim() != 2 or tbox.shape[1] != cols or tcls.numel() != L or timg.numel() != L:
            raise ValueError(f"{who}: tbox must be (L, {cols}){what} with L classes and L image indices")
    return L


def val_match(bufs: NmsBuffers, tbox: torch.Tensor, tcls: torch.Tensor, timg: torch.Tensor, iouv: Sequence[float], clip_wh: Tuple[float, float],
              single_cls: bool = False, want_best: bool = False):
    """The validator's matching (``BaseValidator.match_predictions`` on ``box_iou``, predictions clipped to ``clip_wh``) of a whole batch
    on the padded NMS output through ``dy_val_match``; no host synchronisation.

    ``bufs``: what ``nms`` returned; ``tbox`` (L, 4): the batch's label boxes, xyxy in pixels, clipped; ``tcls`` (L,) their classes and
    ``timg`` (L,) the image each belongs to (any order; converted here, on the device, to the fp32 / int32 the kernel reads); ``iouv``:
    1..16 thresholds (host values, rounded to fp32 as the host comparison rounds them).  Returns ``tp`` uint8 (N, max_det, len(iouv)),
    new tensors on every call; with ``want_best`` ``(tp, best_iou fp32 (N, max_det), best_label int32 (N, max_det))``.  Rows at or
    beyond ``bufs.count`` are 0 / 0 / -1."""
    if _check_labels("val_match", "", 4, tbox, tcls, timg):
        tbox = tbox.to(torch.float32).contiguous()
    return _val_match(lib().dy_val_match, bufs, tbox, tcls, timg, iouv, clip_wh, single_cls, want_best)


def val_match_rotated(bufs: RNmsBuffers, tbox: torch.Tensor, tcls: torch.Tensor, timg: torch.Tensor, iouv: Sequence[float], clip_wh: Tuple[float, float],
                      single_cls: bool = False, want_best: bool = False):
    """The oriented-box validator's matching (``match_predictions`` on ``batch_probiou(gt, det)``, predictions clipped as its ``_prepare_pred``
    clips them) of a whole batch on the padded rotated-NMS output through ``dy_val_match_rotated``; no host synchronisation.

    ``bufs``: what ``nms_rotated`` / ``nms_rotated_ml`` returned; ``tbox`` (L, 5): the batch's labels, xywhr in pixels / radians, already
    scaled and clipped (padded here, on the device, to the kernel's 8 floats per label); ``tcls`` (L,), ``timg`` (L,) (any order); ``iouv``:
    1..16 thresholds.  Returns ``tp`` uint8 (N, max_det, len(iouv)), new tensors on every call; with ``want_best`` ``(tp, best_iou fp32
    (N, max_det), best_label int32 (N, max_det))``.  Rows at or beyond ``bufs.count`` are 0 / 0 / -1."""
    if bufs.out.shape[-1] != 7:
        raise ValueError("val_match_rotated: the NMS buffers must hold 7-column rows (RNmsBuffers)")
    L = _check_labels("val_match_rotated", " xywhr", 5, tbox, tcls, timg)
    if L:
        padded = torch.zeros((L, 8), dtype=torch.float32, device=bufs.out.device)
        padded[:, :5] = tbox
        tbox = padded
    return _val_match(lib().dy_val_match_rotated, bufs, tbox, tcls, timg, iouv, clip_wh, single_cls, want_best)


def val_oks_match(bufs: NmsBuffers, kpts: torch.Tensor, kpt_shape, tbox: torch.Tensor, tkpt: torch.Tensor, tcls: torch.Tensor, timg: torch.Tensor,
                  sigma: Sequence[float], iouv: Sequence[float], clip_wh: Tuple[float, float], nc: Optional[int] = None, single_cls: bool = False,
                  want_best: bool = False):
    """The pose validator's keypoint matching (``match_predictions`` on ``kpt_iou(gt, pred, area = box area * 0.53, sigma)``, predictions
    clipped to ``clip_wh`` as ``scale_coords`` at gain 1 clips them) of a whole batch on the padded NMS output through ``dy_val_oks_match``; no
    host synchronisation, no gather launch.

    ``bufs``: what ``nms`` returned.  ``kpts``, one of two addressings:
      dense plus index  the contiguous fp32 (N, 4 + nc + nk, A) tensor the unfused ``Pose.forward`` returns, with ``nc=`` given: the keypoint
                        channels are read at offset 4 + nc through ``bufs.index``;
      gathered rows     the contiguous fp32 (N, max_det, nk) rows ``kpt_gather`` returns (``nc`` None).
    ``kpt_shape`` = (nkpt, ndim), nkpt <= 32; ``tbox`` (L, 4) the label boxes (xyxy in pixels, clipped), ``tkpt`` (L, nkpt, 3) their keypoints
    (pixels, clipped) and visibilities, ``tcls`` (L,), ``timg`` (L,) (any order); ``sigma``: nkpt host values; ``iouv``: 1..16 thresholds.
    Returns ``tp`` uint8 (N, max_det, len(iouv)), new tensors on every call; with ``want_best`` ``(tp, best_iou, best_label)``.  Rows at or beyond
    ``bufs.count`` are 0 / 0 / -1."""
    nkpt, ndim = int(kpt_shape[0]), int(kpt_shape[1])
    nk = nkpt * ndim
    n, max_det, dev = bufs.batch, bufs.max_det, bufs.out.device
    if nkpt > _lib.OKS_MAX_KPT:
        raise NotImplementedError(f"val_oks_match: {nkpt} keypoints; dy_val_oks_match takes at most {_lib.OKS_MAX_KPT} (the LDS stage)")
    if ndim not in (2, 3) or nkpt < 1 or len(sigma) != nkpt:
        raise ValueError("val_oks_match: kpt_shape must be (nkpt >= 1, 2 | 3) with one sigma per keypoint")
    if bufs.out.shape[-1] != NmsBuffers.ROW:
        raise ValueError("val_oks_match: the NMS buffers must hold 6-column rows (NmsBuffers)")
    require_device(kpts, "keypoints")
    if kpts.dtype != torch.float32 or not kpts.is_contiguous() or kpts.dim() != 3 or kpts.shape[0] != n:
        raise ValueError("val_oks_match: kpts must be a contiguous fp32 (N, 4 + nc + nk, A) or (N, max_det, nk) tensor")
    d = _lib.ValOksMatchDesc()
    if nc is not None:
        if kpts.shape[1] != 4 + nc + nk or kpts.shape[2] != bufs.anchors:
            raise ValueError(f"val_oks_match: the dense form takes (N, {4 + nc + nk}, {bufs.anchors}), got {tuple(kpts.shape)}")
        a = int(kpts.shape[2])
        d.kpts, d.index = kpts.data_ptr() + 4 * (4 + nc) * a, bufs.index.data_ptr()
        d.stride_b, d.stride_ch, d.stride_d, d.anchors = int(kpts.shape[1]) * a, a, 1, a
    else:
        if tuple(kpts.shape[1:]) != (max_det, nk):
            raise ValueError(f"val_oks_match: the gathered form takes (N, {max_det}, {nk}), got {tuple(kpts.shape)}")
        d.kpts, d.index = kpts.data_ptr(), None
        d.stride_b, d.stride_ch, d.stride_d, d.anchors = max_det * nk, 1, nk, 0
    L = _check_labels("val_oks_match", "", 4, tbox, tcls, timg)
    if L:
        require_device(tkpt, "label")
        if tuple(tkpt.shape) != (L, nkpt, 3):
            raise ValueError(f"val_oks_match: tkpt must be (L, {nkpt}, 3): x, y in pixels and the visibility")
        tbox = tbox.to(torch.float32).contiguous()
        tkpt = tkpt.to(torch.float32).contiguous()
        tcls = tcls.reshape(-1).to(torch.float32).contiguous()
        timg = timg.reshape(-1).to(torch.int32).contiguous()
    thr = (C.c_float * len(iouv))(*[float(v) for v in iouv])
    sg = (C.c_float * nkpt)(*[float(v) for v in sigma])
    tp = torch.empty((n, max_det, len(iouv)), dtype=torch.uint8, device=dev)
    best_iou = torch.empty((n, max_det), dtype=torch.float32, device=dev) if want_best else None
    best_label = torch.empty((n, max_det), dtype=torch.int32, device=dev) if want_best else None
    d.rows, d.counts = bufs.out.data_ptr(), bufs.count.data_ptr()
    d.tbox, d.tkpt, d.tcls, d.timg = (tbox.data_ptr(), tkpt.data_ptr(), tcls.data_ptr(), timg.data_ptr()) if L else (None, None, None, None)
    d.sigma, d.iouv = sg, thr
    d.batch, d.max_det, d.n_labels, d.n_iouv, d.nkpt, d.ndim = n, max_det, L, len(iouv), nkpt, ndim
    d.clip_w, d.clip_h, d.single_cls = float(clip_wh[0]), float(clip_wh[1]), int(bool(single_cls))
    d.tp = tp.data_ptr()
    d.best_iou = best_iou.data_ptr() if want_best else None
    d.best_label = best_label.data_ptr() if want_best else None
    _launch(lib().dy_val_oks_match, (C.byref(d),), keep=(d, thr, sg, bufs, kpts, tbox, tkpt, tcls, timg, tp, best_iou, best_label))
    return (tp, best_iou, best_label) if want_best else tp


def label_offsets(timg: torch.Tensor, batch: int) -> torch.Tensor:
    """int32 (batch + 1) exclusive prefix of the labels per image, from the image index of every label, built where ``timg`` lives without a
    host synchronisation (``torch.bincount`` would read the largest index back)."""
    per = torch.zeros((batch + 1,), dtype=torch.int64, device=timg.device)
    if timg.numel():
        per.index_add_(0, timg.reshape(-1).long() + 1, torch.ones((timg.numel(),), dtype=torch.int64, device=timg.device))
    return per.cumsum(0).to(torch.int32)


def val_mask_match_check(proto_hw: Tuple[int, int], map_hw: Tuple[int, int], l_cap: int, n_iouv: int) -> int:
    """The host-side refusals of ``val_mask_match`` (no device needed): returns the grid ratio (1 or 2)."""
    (mh, mw), (gh, gw) = proto_hw, map_hw
    if (mh, mw) == (gh, gw):
        ratio = 1
    elif (mh, mw) == (2 * gh, 2 * gw):
        ratio = 2
    else:
        raise ValueError(f"val_mask_match: the prototype grid {mh} x {mw} must equal the label map's {gh} x {gw} or be exactly twice it on both axes")
    if mh * mw > 1 << 24:
        raise ValueError(f"val_mask_match: a prototype grid of {mh} x {mw} pixels is beyond 2^24 (the pixel counts must stay exact in fp32)")
    if l_cap > _lib.VAL_MASK_MAX_LABELS:
        raise NotImplementedError(f"val_mask_match: {l_cap} labels in one image; dy_val_mask_match takes at most {_lib.VAL_MASK_MAX_LABELS} (one LDS bin each)")
    if not 1 <= n_iouv <= 16:
        raise ValueError("val_mask_match: 1..16 IoU thresholds")
    return ratio


def val_mask_match(bufs: NmsBuffers, protos: torch.Tensor, side: torch.Tensor, label_map: torch.Tensor, tcls: torch.Tensor, timg: torch.Tensor,
                   iouv: Sequence[float], in_wh: Tuple[int, int], l_cap: int, single_cls: bool = False, want_best: bool = False,
                   want_counts: bool = False):
    """The segmentation validator's mask matching of a whole batch through ``dy_val_mask_match`` (``ops.process_mask`` at prototype
    resolution, ``mask_iou`` against the overlap label map, ``match_predictions``); no host synchronisation.

    ``bufs``: what ``nms`` returned; ``protos``: fp32 NHWC view (N, 32, mh, mw); ``side``: ``mask_gather``'s output; ``label_map``: uint8 /
    int32 (N, gh, gw), value k >= 1 = the k-th label of the image; ``tcls`` (L,) and ``timg`` (L,): the batch's label classes and image
    indices, image after image in map order; ``in_wh``: the network input size; ``l_cap``: a host bound on the labels per image (at most
    1024).  Returns ``tp_m`` uint8 (N, max_det, len(iouv)); with ``want_best`` also ``best_iou`` / ``best_label`` (position in ``tcls``);
    with ``want_counts`` also ``inter`` (N, max_det, l_cap), ``area_pred`` (N, max_det), ``area_gt`` (N, l_cap), int32.  New tensors on
    every call; rows at or beyond ``bufs.count`` are 0 / 0 / -1."""
    n, max_det, dev = bufs.batch, bufs.max_det, bufs.out.device
    if protos.dim() != 4 or protos.shape[0] != n or protos.dtype != torch.float32:
        raise ValueError("val_mask_match: protos must be an fp32 (N, nm, mh, mw) NHWC view")
    nm, mh, mw = int(protos.shape[1]), int(protos.shape[2]), int(protos.shape[3])
    if nm != NM:
        raise NotImplementedError(f"val_mask_match: {nm} mask coefficients; dy_val_mask_match is built for {NM}")
    if label_map.dim() != 3 or label_map.shape[0] != n or label_map.dtype not in (torch.uint8, torch.int32):
        raise ValueError("val_mask_match: the label map must be uint8 or int32 (N, gh, gw)")
    l_cap = max(int(l_cap), 1)
    val_mask_match_check((mh, mw), (int(label_map.shape[1]), int(label_map.shape[2])), l_cap, len(iouv))
    if side.dtype != torch.float32 or tuple(side.shape) != (n, max_det, 4 + NM) or not side.is_contiguous():
        raise ValueError("val_mask_match: side must be the contiguous fp32 (N, max_det, 36) output of mask_gather")
    L = int(tcls.numel())
    if timg.numel() != L:
        raise ValueError("val_mask_match: one image index per label class")
    require_device(protos, "protos")
    for t, what in ((side, "side buffer"), (label_map, "label map"), (tcls, "label"), (timg, "label")):
        require_device(t, what)
    label_map = label_map.contiguous()
    tcls = tcls.reshape(-1).to(torch.float32).contiguous()
    loff = label_offsets(timg, n)
    thr = (C.c_float * len(iouv))(*[float(v) for v in iouv])
    tp = torch.empty((n, max_det, len(iouv)), dtype=torch.uint8, device=dev)
    best_iou = torch.empty((n, max_det), dtype=torch.float32, device=dev)
    best_label = torch.empty((n, max_det), dtype=torch.int32, device=dev)
    area_gt = torch.empty((n, l_cap), dtype=torch.int32, device=dev)
    inter = torch.empty((n, max_det, l_cap), dtype=torch.int32, device=dev) if want_counts else None
    area_pred = torch.empty((n, max_det), dtype=torch.int32, device=dev) if want_counts else None
    d = ValMaskMatchDesc()
    d.protos, d.ld_p = view_params(protos)
    d.side, d.rows, d.counts = side.data_ptr(), bufs.out.data_ptr(), bufs.count.data_ptr()
    d.map, d.tcls, d.loff, d.iouv = label_map.data_ptr(), (tcls.data_ptr() if L else None), loff.data_ptr(), thr
    d.batch, d.max_det, d.nm, d.mh, d.mw, d.gh, d.gw = n, max_det, nm, mh, mw, int(label_map.shape[1]), int(label_map.shape[2])
    d.map_dtype = _lib.DY_MAP_U8 if label_map.dtype == torch.uint8 else _lib.DY_MAP_I32
    d.n_labels, d.l_cap, d.n_iouv = L, l_cap, len(iouv)
    d.in_w, d.in_h, d.single_cls = int(in_wh[0]), int(in_wh[1]), int(bool(single_cls))
    d.tp_m, d.best_iou, d.best_label, d.area_gt = tp.data_ptr(), best_iou.data_ptr(), best_label.data_ptr(), area_gt.data_ptr()
    d.inter = inter.data_ptr() if want_counts else None
    d.area_pred = area_pred.data_ptr() if want_counts else None
    _launch(lib().dy_val_mask_match, (C.byref(d),), keep=(d, thr, bufs, protos, side, label_map, tcls, loff, tp, best_iou, best_label, area_gt, inter, area_pred))
    out = (tp,)
    if want_best:
        out += (best_iou, best_label)
    if want_counts:
        out += (inter, area_pred, area_gt)
    return out if len(out) > 1 else tp


# ---- tracking ---------------------------------------------------------------------------------------------


class TrackBuffers:
    """Persistent state, workspace and outputs of ``dy_track_step`` for (streams, max_tracks, max_det).  ``out`` / ``count`` grow with the
    largest batch seen; the state lives as long as the object (``track_reset`` empties it).  ``rotated``: the buffers of
    ``dy_track_step_rotated`` (7-float detection rows in, 9-float rows out, a state with the angle per slot)."""

    def __init__(self, streams: int, max_tracks: int, max_det: int, device, rotated: bool = False):
        self.streams, self.max_tracks, self.max_det, self.device = int(streams), int(max_tracks), int(max_det), torch.device(device)
        self.rotated = bool(rotated)
        self.suffix = "_rotated" if self.rotated else ""
        self.row_in, self.row_out = (7, 9) if self.rotated else (6, 8)
        nstate = getattr(lib(), "dy_track_state_bytes" + self.suffix)(self.streams, self.max_tracks)
        nws = getattr(lib(), "dy_track_workspace_bytes" + self.suffix)(self.streams, self.max_tracks, self.max_det)
        if nstate < 0 or nws < 0:
            check(int(min(nstate, nws)), f"dy_track_state_bytes{self.suffix} / dy_track_workspace_bytes{self.suffix}")
        self.state = torch.zeros((nstate,), dtype=torch.uint8, device=self.device)
        self.workspace = torch.empty((nws,), dtype=torch.uint8, device=self.device)
        self.out: Optional[torch.Tensor] = None
        self.count: Optional[torch.Tensor] = None

    def outputs(self, images: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.out is None or self.out.shape[0] < images:
            self.out = torch.empty((images, self.max_tracks, self.row_out), dtype=torch.float32, device=self.device)
            self.count = torch.empty((images,), dtype=torch.int32, device=self.device)
        return self.out[:images], self.count[:images]


def track_reset(bufs: TrackBuffers) -> None:
    """No tracks, frame and id counters 0 (``BYTETracker.reset``), stream-ordered."""
    _launch(getattr(lib(), "dy_track_reset" + bufs.suffix), (bufs.state.data_ptr(), bufs.streams, bufs.max_tracks), keep=(bufs,), record=False)


def track_counters(bufs: TrackBuffers):
    """(streams, 3) int32 on the host: frame counter, id counter, overflow counter of every stream (synchronises)."""
    per = bufs.state.numel() // bufs.streams
    return bufs.state.view(bufs.streams, per)[:, :12].contiguous().view(torch.int32).cpu().numpy()


def track_step(bufs: TrackBuffers, nms_bufs, frames: int, streams: int, cfg, max_time_lost: Optional[int] = None, frame_rate: int = 30):
    """ByteTrack over ``frames`` time steps of ``streams`` video streams in one ``dy_track_step`` launch; no host synchronisation.
    ``nms_bufs``: ``NmsBuffers`` (after ``scale_boxes_``) or a ``(rows, counts)`` pair of device tensors, (frames * streams, max_det, 6)
    fp32 / int32; ``cfg``: the tracker settings (``trackers.load_tracker_cfg``).  Returns views ``(out (frames * streams, max_tracks, 8),
    count (frames * streams,))`` of ``bufs``' output tensors: rows [x1, y1, x2, y2, id, score, cls, idx] in ascending id.  With rotated
    buffers (``RNmsBuffers`` after ``scale_rboxes_``): rows (.., max_det, 7) [x, y, w, h, r, conf, cls] through ``dy_track_step_rotated``,
    out (.., max_tracks, 9) [x, y, w, h, r, id, score, cls, idx]."""
    rows, counts = (nms_bufs.out, nms_bufs.count) if hasattr(nms_bufs, "out") else nms_bufs
    require_device(rows, "detection rows")
    require_device(counts, "detection counts")
    n = int(frames) * int(streams)
    if streams != bufs.streams or rows.dtype != torch.float32 or counts.dtype != torch.int32 or not rows.is_contiguous() or not counts.is_contiguous() \
            or tuple(rows.shape) != (n, bufs.max_det, bufs.row_in) or counts.numel() != n:
        raise ValueError(f"track_step: rows must be contiguous fp32 ({n}, {bufs.max_det}, {bufs.row_in}) with {n} int32 counts for {bufs.streams} streams")
    out, cnt = bufs.outputs(n)
    d = TrackDesc()
    d.rows, d.counts = rows.data_ptr(), counts.data_ptr()
    d.state, d.state_bytes, d.workspace, d.workspace_bytes = bufs.state.data_ptr(), bufs.state.numel(), bufs.workspace.data_ptr(), bufs.workspace.numel()
    d.out, d.out_count = out.data_ptr(), cnt.data_ptr()
    d.frames, d.streams, d.max_det, d.max_tracks = int(frames), int(streams), bufs.max_det, bufs.max_tracks
    d.track_high_thresh, d.track_low_thresh, d.new_track_thresh = float(cfg.track_high_thresh), float(cfg.track_low_thresh), float(cfg.new_track_thresh)
    d.match_thresh, d.fuse_score = float(cfg.match_thresh), int(bool(cfg.fuse_score))
    d.max_time_lost = int(frame_rate / 30.0 * cfg.track_buffer) if max_time_lost is None else int(max_time_lost)
    _launch(getattr(lib(), "dy_track_step" + bufs.suffix), (C.byref(d),), keep=(d, bufs, rows, counts), record=False)
    return out, cnt


# ---- training loss (forward) ----------------------------------------------------------------------------


def detection_loss(levels: Sequence[torch.Tensor], gt: torch.Tensor, strides: Sequence[float], nc: int, reg_max: int = 16,
                   topk: int = 10, alpha: float = 0.5, beta: float = 6.0, box: float = 7.5, cls: float = 0.5, dfl: float = 1.5,
                   want_owner: bool = False, want_grad: bool = False):
    """v8DetectionLoss forward through ``dy_detection_loss``.

    levels[i]: fp32 NHWC view (N, 4*reg_max+nc, H_i, W_i) — Detect's training-mode outputs; gt: device fp32 (N, gmax, 5)
    [cls, x1, y1, x2, y2] in pixels, zero rows = padding.  Returns (out[4] = box, cls, dfl, total, owner or None) and,
    with ``want_grad``, a third item: the list of d total / d levels[i] (fp32 NHWC views shaped like the inputs)."""
    n = levels[0].shape[0]
    d = LossDesc()
    A = 0
    for i, t in enumerate(levels):
        require_device(t)
        if t.dtype != torch.float32 or t.shape[1] != 4 * reg_max + nc:
            raise ValueError("detection_loss: levels must be fp32 with 4*reg_max+nc channels")
        p_, ld = view_params(t)
        d.level[i], d.h[i], d.w[i], d.ld[i], d.stride[i] = p_, t.shape[2], t.shape[3], ld, float(strides[i])
        A += t.shape[2] * t.shape[3]
    dev = levels[0].device
    gt = gt.to(dev, torch.float32).contiguous()
    if gt.dim() != 3 or gt.shape[0] != n or gt.shape[2] != 5:
        raise ValueError("detection_loss: gt must be (N, gmax, 5)")
    gmax = gt.shape[1]
    d.n_levels, d.batch, d.nc, d.reg_max = len(levels), n, nc, reg_max
    d.gt, d.gmax, d.topk = (gt.data_ptr() if gmax else None), gmax, topk
    d.alpha, d.beta, d.box_gain, d.cls_gain, d.dfl_gain = alpha, beta, box, cls, dfl
    out = torch.empty(4, dtype=torch.float32, device=dev)
    owner = torch.empty((n, A), dtype=torch.int32, device=dev) if want_owner else None
    ws = torch.empty(lib().dy_detection_loss_workspace_bytes(n, A, gmax, topk), dtype=torch.uint8, device=dev)
    d.out, d.out_owner = out.data_ptr(), (owner.data_ptr() if want_owner else None)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    grads = None
    if want_grad:
        grads = []
        for i, t in enumerate(levels):
            gt_ = alloc_nhwc(n, t.shape[1], t.shape[2], t.shape[3], torch.float32, dev, ld=d.ld[i])
            d.grad_level[i], d.ld_grad[i] = view_params(gt_)
            grads.append(gt_)
    _launch(lib().dy_detection_loss, (C.byref(d),), keep=(d, out, owner, ws, gt, *levels, *(grads or ())))
    return (out, owner, grads) if want_grad else (out, owner)


def obb_loss(levels: Sequence[torch.Tensor], angles: Sequence[torch.Tensor], gt: torch.Tensor, strides: Sequence[float], nc: int, reg_max: int = 16,
             topk: int = 10, alpha: float = 0.5, beta: float = 6.0, box: float = 7.5, cls: float = 0.5, dfl: float = 1.5,
             want_owner: bool = False, want_grad: bool = False, buffers: Optional[dict] = None):
    """v8OBBLoss forward (and gradient) through ``dy_obb_loss``.

    levels[i]: fp32 NHWC view (N, 4*reg_max+nc, H_i, W_i); angles[i]: fp32 NHWC view (N, >=1, H_i, W_i) whose channel 0 is the raw angle
    logit; gt: fp32 (N, gmax, 6) [cls, x, y, w, h, r], pixels and radians, zero rows = padding, on the host or the device.  Returns
    (out[4] = box, cls, dfl, total, owner or None) and, with ``want_grad``, two more items: d total / d levels[i] and d total / d angles[i]
    (NHWC views shaped and pitched like the inputs; the angle gradient's channel 0 carries the value, the others zeros).  ``buffers``: a
    dict the call fills on first use and reuses afterwards (out, owner, workspace, gradient maps) -- static buffers, as under graph replay."""
    n = levels[0].shape[0]
    if len(angles) != len(levels):
        raise ValueError("obb_loss: one angle map per level")
    d = ObbLossDesc()
    A = 0
    for i, (t, an) in enumerate(zip(levels, angles)):
        require_device(t)
        require_device(an)
        if t.dtype != torch.float32 or t.shape[1] != 4 * reg_max + nc:
            raise ValueError("obb_loss: levels must be fp32 with 4*reg_max+nc channels")
        if an.dtype != torch.float32 or an.shape[0] != n or an.shape[1] < 1 or an.shape[2:] != t.shape[2:]:
            raise ValueError("obb_loss: angles must be fp32 maps of the levels' sizes")
        p_, ld = view_params(t)
        d.level[i], d.h[i], d.w[i], d.ld[i], d.stride[i] = p_, t.shape[2], t.shape[3], ld, float(strides[i])
        d.angle[i], d.ld_angle[i] = view_params(an)
        A += t.shape[2] * t.shape[3]
    dev = levels[0].device
    gt = gt.to(dev, torch.float32).contiguous()
    if gt.dim() != 3 or gt.shape[0] != n or gt.shape[2] != 6:
        raise ValueError("obb_loss: gt must be (N, gmax, 6)")
    gmax = gt.shape[1]
    d.n_levels, d.batch, d.nc, d.reg_max = len(levels), n, nc, reg_max
    d.gt, d.gmax, d.topk = (gt.data_ptr() if gmax else None), gmax, topk
    d.alpha, d.beta, d.box_gain, d.cls_gain, d.dfl_gain = alpha, beta, box, cls, dfl
    bufs = buffers if buffers is not None else {}
    if "out" not in bufs:
        bufs["out"] = torch.empty(4, dtype=torch.float32, device=dev)
        bufs["owner"] = torch.empty((n, A), dtype=torch.int32, device=dev) if want_owner else None
        bufs["ws"] = torch.empty(lib().dy_obb_loss_workspace_bytes(n, A, gmax, topk), dtype=torch.uint8, device=dev)
        bufs["grads"] = bufs["agrads"] = None
        if want_grad:
            bufs["grads"] = [alloc_nhwc(n, t.shape[1], t.shape[2], t.shape[3], torch.float32, dev, ld=d.ld[i]) for i, t in enumerate(levels)]
            bufs["agrads"] = [alloc_nhwc(n, an.shape[1], an.shape[2], an.shape[3], torch.float32, dev, ld=d.ld_angle[i]) for i, an in enumerate(angles)]
    out, owner, ws, grads, agrads = bufs["out"], bufs["owner"], bufs["ws"], bufs["grads"], bufs["agrads"]
    d.out, d.out_owner = out.data_ptr(), (owner.data_ptr() if owner is not None else None)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if want_grad:
        for i in range(len(levels)):
            d.grad_level[i], d.ld_grad[i] = view_params(grads[i])
            d.grad_angle[i], d.ld_grad_angle[i] = view_params(agrads[i])
    _launch(lib().dy_obb_loss, (C.byref(d),), keep=(d, out, owner, ws, gt, *levels, *angles, *(grads or ()), *(agrads or ())))
    return (out, owner, grads, agrads) if want_grad else (out, owner)


def seg_loss(owner: torch.Tensor, gt: torch.Tensor, coefs: Sequence[torch.Tensor], proto: torch.Tensor, masks: torch.Tensor, img_hw, box: float = 7.5,
             topk: int = 10, want_grad: bool = False, buffers: Optional[dict] = None):
    """The mask term of v8SegmentationLoss (and its gradient) through ``dy_seg_loss``, behind ``detection_loss(..., want_owner=True)``.

    owner: int32 (N, A) from ``detection_loss``; gt: its fp32 (N, gmax, 5) table; coefs[i]: fp32 NHWC views (N, 32, h_i, w_i) of Segment.cv4;
    proto: an NHWC view (N, 32, mh, mw) in bf16, f16 or fp32; masks: uint8 or int32 (N, gh, gw) overlap index maps (value k + 1 = row k of the
    image in ``gt``) with (mh, mw) = (gh, gw) or exactly twice it; img_hw = (h, w) of the input in pixels.  Every argument is checked here, on the
    host, before any launch.  Returns ``out`` (fp32[2] = seg, seg * N) and, with ``want_grad``, the fp32 gradient maps of d (seg * N): one per
    coefficient level (shape and pitch of ``coefs[i]``) and the prototypes' (N, 32, mh, mw).  ``buffers``: a dict the call fills on first use
    and reuses afterwards (out, workspace, gradient maps)."""
    require_device(owner, "seg_loss owner")
    require_device(proto, "seg_loss proto")
    if not isinstance(masks, torch.Tensor) or masks.dtype not in (torch.uint8, torch.int32):
        raise TypeError(f"seg_loss: masks must be uint8 or int32 overlap index maps (overlap_mask=True), got {getattr(masks, 'dtype', type(masks).__name__)}")
    n, nm, mh, mw = proto.shape
    if nm != NM or any(t.shape[1] != NM for t in coefs):
        raise NotImplementedError(f"seg_loss: built for nm = {NM} mask coefficients, got {nm}")
    if masks.dim() != 3 or masks.shape[0] != n:
        raise ValueError(f"seg_loss: masks must be (N, gh, gw) index maps, got {tuple(masks.shape)}")
    gh, gw = int(masks.shape[1]), int(masks.shape[2])
    if (mh, mw) != (gh, gw) and (mh, mw) != (2 * gh, 2 * gw):
        raise ValueError(f"seg_loss: the prototype grid {mh} x {mw} must equal the index map's {gh} x {gw} or be exactly twice it on both axes")
    if proto.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError(f"seg_loss: prototypes must be bfloat16, float16 or float32, got {proto.dtype}")
    dev = proto.device
    A = sum(t.shape[2] * t.shape[3] for t in coefs)
    if owner.dtype != torch.int32 or tuple(owner.shape) != (n, A) or not owner.is_contiguous():
        raise ValueError(f"seg_loss: owner must be a contiguous int32 ({n}, {A}) map")
    gt = gt.to(dev, torch.float32).contiguous()
    if gt.dim() != 3 or gt.shape[0] != n or gt.shape[2] != 5:
        raise ValueError("seg_loss: gt must be (N, gmax, 5)")
    gmax = gt.shape[1]
    if masks.dtype == torch.uint8 and gmax > 255:
        raise ValueError(f"seg_loss: {gmax} label rows do not fit a uint8 index map; pass int32 maps")
    masks = masks.to(dev).contiguous()
    d = SegLossDesc()
    for i, t in enumerate(coefs):
        require_device(t)
        if t.dtype != torch.float32 or t.shape[0] != n:
            raise ValueError("seg_loss: coefficient maps must be fp32 (N, 32, h, w)")
        d.coef[i], d.ld_coef[i] = view_params(t)
        d.h[i], d.w[i] = t.shape[2], t.shape[3]
    d.owner, d.gt = owner.data_ptr(), (gt.data_ptr() if gmax else None)
    d.n_levels, d.batch, d.nm, d.gmax, d.topk = len(coefs), n, nm, gmax, topk
    d.proto, d.ld_proto = view_params(proto)
    d.proto_dtype, d.mh, d.mw = dy_dtype(proto.dtype), mh, mw
    d.masks, d.mask_dtype, d.gh, d.gw = masks.data_ptr(), (1 if masks.dtype == torch.int32 else 0), gh, gw
    d.img_h, d.img_w, d.box_gain = float(img_hw[0]), float(img_hw[1]), box
    bufs = buffers if buffers is not None else {}
    if "out" not in bufs:
        bufs["out"] = torch.empty(2, dtype=torch.float32, device=dev)
        bufs["ws"] = torch.empty(lib().dy_seg_loss_workspace_bytes(n, A, gmax, topk), dtype=torch.uint8, device=dev)
        bufs["gcoef"] = bufs["gproto"] = None
        if want_grad:
            bufs["gcoef"] = [alloc_nhwc(n, NM, t.shape[2], t.shape[3], torch.float32, dev, ld=d.ld_coef[i]) for i, t in enumerate(coefs)]
            bufs["gproto"] = alloc_nhwc(n, NM, mh, mw, torch.float32, dev)
    out, ws, gcoef, gproto = bufs["out"], bufs["ws"], bufs["gcoef"], bufs["gproto"]
    d.out, d.workspace, d.workspace_bytes = out.data_ptr(), ws.data_ptr(), ws.numel()
    if want_grad:
        for i in range(len(coefs)):
            d.grad_coef[i], d.ld_grad_coef[i] = view_params(gcoef[i])
        d.grad_proto, d.ld_grad_proto = view_params(gproto)
    _launch(lib().dy_seg_loss, (C.byref(d),), keep=(d, out, ws, owner, gt, masks, proto, *coefs, *(gcoef or ()), gproto))
    return (out, gcoef, gproto) if want_grad else out


# ---- train-mode BatchNorm (+ SiLU) -------------------------------------------------------------------------------


class BnState:
    """Saved batch statistics + workspace of one BatchNorm layer for one training step."""

    def __init__(self, c: int, device):
        self.c = c
        self.mean = torch.empty(c, dtype=torch.float32, device=device)
        self.rstd = torch.empty(c, dtype=torch.float32, device=device)
        self.ws = torch.empty(lib().dy_bn_workspace_bytes(c), dtype=torch.uint8, device=device)


def _rows(t: torch.Tensor) -> int:
    return t.shape[0] * t.shape[2] * t.shape[3]


def bn_train_fwd(z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, state: BnState, act: bool, eps: float = 1e-3,
                 momentum: float = 0.03, running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None,
                 addend: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, partial_slabs: int = 0) -> torch.Tensor:
    """y = act(BN_batchstats(z) (+ addend)) through ``dy_bn_train_fwd``; z, y, addend: NHWC views (N, C, H, W).
    ``partial_slabs``: > 0 = ``state``'s workspace already holds that many partial-sum slots of z (``conv2d(bn_stats=state)``): no reduction pass."""
    require_device(z, "bn input")
    n, c, h, w = z.shape
    if out is None:
        out = alloc_nhwc(n, c, h, w, z.dtype, z.device)
    d = BnDesc()
    (d.z, d.ld_z), (d.y, d.ld_y) = view_params(z), view_params(out)
    if addend is not None:
        d.addend, d.ld_add = view_params(addend)
    d.rows, d.c, d.dtype, d.act = _rows(z), c, dy_dtype(z.dtype), DY_ACT_SILU if act else DY_ACT_NONE
    d.gamma, d.beta, d.mean, d.rstd = gamma.data_ptr(), beta.data_ptr(), state.mean.data_ptr(), state.rstd.data_ptr()
    if running_mean is not None:
        d.running_mean, d.running_var = running_mean.data_ptr(), running_var.data_ptr()
    d.eps, d.momentum = eps, momentum
    d.workspace, d.workspace_bytes = state.ws.data_ptr(), state.ws.numel()
    d.partial_slabs = int(partial_slabs)
    _launch(lib().dy_bn_train_fwd, (C.byref(d),), keep=(d, z, out, addend, gamma, beta, state, running_mean, running_var))
    return out


def bn_train_bwd(dy: torch.Tensor, z: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, state: BnState, act: bool,
                 dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 partial_slabs: int = 0):
    """(dz, dgamma, dbeta) of y = act(BN_batchstats(z)) given dy, through ``dy_bn_train_bwd`` (state from the forward).
    ``partial_slabs``: > 0 = the workspace already holds that many slots of the sums of du and du * xhat (``BnBehind.slots``): no reduction pass."""
    n, c, h, w = z.shape
    if out is None:
        out = alloc_nhwc(n, c, h, w, z.dtype, z.device)
    if dgamma is None:
        dgamma = torch.empty(c, dtype=torch.float32, device=z.device)
    if dbeta is None:
        dbeta = torch.empty(c, dtype=torch.float32, device=z.device)
    d = BnDesc()
    (d.z, d.ld_z), (d.dy, d.ld_dy), (d.dz, d.ld_dz) = view_params(z), view_params(dy), view_params(out)
    d.rows, d.c, d.dtype, d.act = _rows(z), c, dy_dtype(z.dtype), DY_ACT_SILU if act else DY_ACT_NONE
    d.gamma, d.beta, d.mean, d.rstd = gamma.data_ptr(), beta.data_ptr(), state.mean.data_ptr(), state.rstd.data_ptr()
    d.dgamma, d.dbeta = dgamma.data_ptr(), dbeta.data_ptr()
    d.workspace, d.workspace_bytes = state.ws.data_ptr(), state.ws.numel()
    d.partial_slabs = int(partial_slabs)
    _launch(lib().dy_bn_train_bwd, (C.byref(d),), keep=(d, z, dy, out, gamma, beta, state, dgamma, dbeta))
    return out, dgamma, dbeta


def silu_fwd(u: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    n, c, h, w = u.shape
    if out is None:
        out = alloc_nhwc(n, c, h, w, u.dtype, u.device)
    (up, ldu), (op, ldo) = view_params(u), view_params(out)
    _launch(lib().dy_silu_fwd, (up, op, _rows(u), c, ldu, ldo, dy_dtype(u.dtype)), keep=(u, out))
    return out


def silu_bwd(u: torch.Tensor, dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    n, c, h, w = u.shape
    if out is None:
        out = alloc_nhwc(n, c, h, w, u.dtype, u.device)
    (up, ldu), (dp, ldd), (op, ldo) = view_params(u), view_params(dy), view_params(out)
    _launch(lib().dy_silu_bwd, (up, dp, op, _rows(u), c, ldu, ldd, ldo, dy_dtype(u.dtype)), keep=(u, dy, out))
    return out


# ---- convolution gradients ----------------------------------------------------------------------------------------


# ---- weight gradients beside the input gradients (r03) -------------------------------------------------------------------
# In the backward of a layer the weight gradient (x, dz -> dw) feeds nothing but the parameter's gradient, while the input gradient
# (dz, w -> dx) is what the rest of the backward waits for.  The wgrad kernels are bound by their closing fp32 atomics and by latency
# (150 - 420 TFLOP/s), the dgrad / BatchNorm kernels by MFMA and HBM: issued on a SECOND stream (forked after dz exists, joined before
# the gradients are read) the two can overlap; inside the captured step graph a fork / join becomes parallel branches.
# MEASURED (r03, B = 64, graphed step): 37.5 ms with everything on one stream, 38.4 - 40.5 ms with the weight gradients on the side
# stream — the hipGraph's branches do not run beside each other to any advantage (the wgrad atomics and the BatchNorm passes contend
# for the same memory pipeline) — so it is OFF unless DYOLO_WGRAD_SIDE=1 asks for it.
_WGRAD_SIDE = {"on": os.environ.get("DYOLO_WGRAD_SIDE", "0") == "1", "streams": {}, "used": False}


def _side_stream(device) -> "torch.cuda.Stream":
    st = _WGRAD_SIDE["streams"].get(str(device))
    if st is None:
        st = _WGRAD_SIDE["streams"][str(device)] = torch.cuda.Stream(device=device)
    return st


def join_side_stream(device=None) -> None:
    """Make the current stream wait for every weight-gradient kernel issued on the side stream (call before the gradients / the sink are
    read: the sink flush, a bucket's flush, the optimizer)."""
    if not _WGRAD_SIDE["used"]:
        return
    for st in _WGRAD_SIDE["streams"].values():
        torch.cuda.current_stream(st.device).wait_stream(st)
    _WGRAD_SIDE["used"] = False


def conv_wgrad_into(x: torch.Tensor, dz: torch.Tensor, ksize: int, stride: int, pad: int, out: torch.Tensor) -> None:
    """``conv_wgrad(..., out=out)`` on the side stream (see above) when that is enabled; ``out`` must be a buffer nobody reads before
    ``join_side_stream`` (a trainer's gradient sink)."""
    if not _WGRAD_SIDE["on"]:
        conv_wgrad(x, dz, ksize, stride, pad, out=out)
        return
    side = _side_stream(x.device)
    side.wait_stream(torch.cuda.current_stream(x.device))  # x and dz exist
    with torch.cuda.stream(side):
        conv_wgrad(x, dz, ksize, stride, pad, out=out)
    x.record_stream(side)  # the allocator must not hand their memory out again before the side stream is past this point
    dz.record_stream(side)
    _WGRAD_SIDE["used"] = True


def conv_wgrad(x: torch.Tensor, dz: torch.Tensor, ksize: int, stride: int, pad: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d loss / d weight of z = conv2d(x, w, stride, pad): fp32 (cout, cin, k, k), through ``dy_conv2d_wgrad_nhwc``.
    ``out``: a contiguous fp32 (cout, k, k, cin) tensor the kernel ADDS into (a trainer's gradient sink) instead of a fresh zeroed one."""
    require_device(x, "wgrad input")
    n, cin, h, w = x.shape
    cout, ho, wo = dz.shape[1], dz.shape[2], dz.shape[3]
    if (ho, wo) != conv_out_hw(h, w, ksize, stride, pad) or dz.shape[0] != n or dz.dtype != x.dtype:
        raise ValueError("conv_wgrad: dz does not match the forward geometry / dtype")
    d = ConvDesc()
    (d.x, d.ld_x), (dzp, lddz) = view_params(x), view_params(dz)
    d.batch, d.h, d.w_in, d.cin, d.ho, d.wo, d.cout = n, h, w, cin, ho, wo, cout
    d.ksize, d.stride, d.pad, d.groups, d.dtype = ksize, stride, pad, 1, dy_dtype(x.dtype)
    if out is not None:
        if tuple(out.shape) != (cout, ksize, ksize, cin) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("conv_wgrad: out must be a contiguous fp32 (cout, k, k, cin) tensor")
        dw = out
    else:
        dw = torch.zeros((cout, ksize, ksize, cin), dtype=torch.float32, device=x.device)
    need = lib().dy_conv2d_wgrad_workspace_bytes(C.byref(d), lddz)
    if need < 0:
        check(int(need), "dy_conv2d_wgrad_workspace_bytes")
    ws = _wgrad_workspace(x.device, need) if need else None
    _launch(lib().dy_conv2d_wgrad_nhwc_ws, (C.byref(d), dzp, lddz, dw.data_ptr(), ws.data_ptr() if need else None, ws.numel() if need else 0),
            keep=(d, x, dz, dw, ws))
    return dw.permute(0, 3, 1, 2)


_WGRAD_WS: dict = {}
_WGRAD_WS_RETIRED: list = []


def _wgrad_workspace(device, need: int) -> torch.Tensor:
    """Scratch of ``dy_conv2d_wgrad_nhwc_ws`` (the 3x3 kernel's per-slab partial sums, <= ~40 MB at any shape): one buffer per
    (device, stream) -- calls that share it are ordered on that stream -- grown on demand and never shrunk."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            _WGRAD_WS_RETIRED.append(ws)  # a captured step graph may still replay launches that write the smaller buffer: it stays allocated
        ws = _WGRAD_WS[key] = torch.empty(max(need, 48 << 20), dtype=torch.uint8, device=device)
    return ws


def conv_grouped_bwd(x: torch.Tensor, dz: torch.Tensor, weight: torch.Tensor, stride: int, pad: int, groups: int, need_dx: bool = True):
    """(dw, dx) of z = conv2d(x, weight, stride, pad, groups=groups) given dz through ``dy_conv2d_grouped_bwd_nhwc``.
    weight: the fp32 master tensor (cout, cin/groups, k, k) on the device; dw comes back in the same layout (fp32)."""
    require_device(x, "grouped wgrad input")
    n, cin, h, w = x.shape
    cout, ho, wo = dz.shape[1], dz.shape[2], dz.shape[3]
    k = weight.shape[2]
    if (ho, wo) != conv_out_hw(h, w, k, stride, pad) or dz.shape[0] != n or dz.dtype != x.dtype or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise ValueError("conv_grouped_bwd: dz / weight do not match the forward geometry, dtype or layout")
    d = ConvDesc()
    (d.x, d.ld_x), (dzp, lddz) = view_params(x), view_params(dz)
    d.batch, d.h, d.w_in, d.cin, d.ho, d.wo, d.cout = n, h, w, cin, ho, wo, cout
    d.ksize, d.stride, d.pad, d.groups, d.dtype = k, stride, pad, groups, dy_dtype(x.dtype)
    dw = torch.zeros_like(weight)
    dx = alloc_nhwc(n, cin, h, w, x.dtype, x.device) if need_dx else None
    dxp, lddx = view_params(dx) if need_dx else (None, 0)
    _launch(lib().dy_conv2d_grouped_bwd_nhwc, (C.byref(d), dzp, lddz, weight.data_ptr(), dw.data_ptr(), dxp, lddx, None, 0), keep=(d, x, dz, weight, dw, dx))
    return dw, dx


def colsum(z: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-channel sum over (N, H, W) of an NHWC view: the bias gradient of a plain convolution.  ``out``: a contiguous fp32 (c,) tensor
    the sums are ADDED to (a trainer's gradient sink) instead of a fresh zeroed one."""
    zp, ld = view_params(z)
    if out is None:
        out = torch.zeros(z.shape[1], dtype=torch.float32, device=z.device)
    elif out.dtype != torch.float32 or out.numel() != z.shape[1] or not out.is_contiguous():
        raise ValueError("colsum: out must be a contiguous fp32 (c,) tensor")
    _launch(lib().dy_colsum, (zp, out.data_ptr(), _rows(z), z.shape[1], ld, dy_dtype(z.dtype)), keep=(z, out))
    return out


def pack_dgrad(weight: torch.Tensor, stride: int, dtype: torch.dtype, device, no_accumulate: bool = False) -> PackedConv:
    """Weights of the convolution that computes dx from dz: w'[ci][co][r][q] = w[co][ci][k-1-r][k-1-q], stride 1,
    pad k-1-pad (= pad for the 'same' convolutions of this model); stride-2 layers run on the generic / LDS-DMA kernels
    (zero-dilated gather), stride-1 3x3 layers may take the halo kernel.  Device-resident fp32 weights (training) are
    transposed, flipped, cast and laid out by one ``dy_pack_conv_weights`` launch."""
    k = weight.shape[2]
    # the streaming 1x1 kernel has no residual (accumulate) input: 1x1 layers take it only when the caller adds nothing in the epilogue
    halo = None if (stride == 1 and (k == 3 or (k == 1 and no_accumulate))) else False
    if weight.is_cuda and weight.dtype == torch.float32 and dtype != FP8 and weight.device == torch.device(device):
        return PackedConv(weight, zero_bias(weight.shape[1], weight.device), 1, k // 2, 1, False, dtype, device, halo=halo, transpose_flip=True)
    wt = weight.detach().permute(1, 0, 2, 3)  # a view: the packing copy below does the layout change
    if k > 1:
        wt = wt.flip(2, 3)
    return PackedConv(wt, zero_bias(wt.shape[0], wt.device), 1, k // 2, 1, False, dtype, device, halo=halo)


def conv_dgrad(dz: torch.Tensor, pc: PackedConv, stride: int, out: Optional[torch.Tensor] = None,
               accumulate: Optional[torch.Tensor] = None, bn_behind: Optional[BnBehind] = None) -> torch.Tensor:
    """dx of z = conv2d(x, w, stride, k//2) given dz, with ``pc = pack_dgrad(w, stride, ...)``; ``accumulate``: a gradient
    already held for x (another consumer's contribution), added in the epilogue; ``bn_behind``: see ``BnBehind`` (x is the output of a
    BatchNorm + activation layer with no other consumer: the sums of its backward come out of this kernel's epilogue where built)."""
    if stride not in (1, 2):
        raise NotImplementedError("conv_dgrad: stride 1 or 2")
    if bn_behind is not None and (accumulate is not None or dz.dtype not in (torch.bfloat16, torch.float16)):
        bn_behind = None  # (its slots stay 0: the BatchNorm backward reduces by itself)
    return conv2d(dz, pc, out=out, residual=accumulate, dil2=(stride == 2), bn_behind=bn_behind)


# ---- small training-path ops + optimizer --------------------------------------------------------------------------


def upsample2x_bwd(g: torch.Tensor) -> torch.Tensor:
    n, c, h2, w2 = g.shape
    out = alloc_nhwc(n, c, h2 // 2, w2 // 2, g.dtype, g.device)
    (gp, ldg), (op, ldo) = view_params(g), view_params(out)
    _launch(lib().dy_upsample2x_bwd_nhwc, (gp, op, n, h2 // 2, w2 // 2, c, ldg, ldo, dy_dtype(g.dtype)), keep=(g, out))
    return out


def maxpool_bwd(x: torch.Tensor, g_out: torch.Tensor, g_in: torch.Tensor, k: int, accumulate: bool) -> torch.Tensor:
    """g_in (+)= gradient of max_pool2d(x, k, 1, k//2) given g_out; all NHWC views of one dtype."""
    n, c, h, w = x.shape
    (xp, ldx), (gop, ldgo), (gip, ldgi) = view_params(x), view_params(g_out), view_params(g_in)
    _launch(lib().dy_maxpool_bwd_nhwc, (xp, gop, gip, n, h, w, c, ldx, ldgo, ldgi, k, int(accumulate), dy_dtype(x.dtype)), keep=(x, g_out, g_in))
    return g_in


def add_dilated2_(dx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """dx[:, :, ::2, ::2] += t in place (``dy_add_dilated2_nhwc``): NHWC views of one dtype, t (n, c, ceil(H/2), ceil(W/2))."""
    n, c, h2, w2 = dx.shape
    if t.shape[0] != n or t.shape[1] != c or t.shape[2] != (h2 + 1) // 2 or t.shape[3] != (w2 + 1) // 2 or t.dtype != dx.dtype:
        raise ValueError("add_dilated2_: t must be the half-resolution map of dx")
    (tp, ldt), (xp, ldx) = view_params(t), view_params(dx)
    _launch(lib().dy_add_dilated2_nhwc, (tp, xp, n, t.shape[2], t.shape[3], h2, w2, c, ldt, ldx, dy_dtype(dx.dtype)), keep=(t, dx))
    return dx


def head_grad_split(g: torch.Tensor, nb: int, nc: int, ncp: int, dtype: torch.dtype, scale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dzb, dzc) of ``dy_head_grad_split``: ``g`` an fp32 NHWC view (n, nb + nc, h, w); ``scale`` a device fp32 scalar or None."""
    n, c, h, w = g.shape
    if g.dtype != torch.float32 or c != nb + nc or g.stride(1) != 1:
        raise ValueError("head_grad_split: g must be an fp32 NHWC view of nb + nc channels")
    gp, ldg = view_params(g)
    dzb, dzc = alloc_nhwc(n, nb, h, w, dtype, g.device), alloc_nhwc(n, ncp, h, w, dtype, g.device)
    (bp, ldb), (cp, ldc) = view_params(dzb), view_params(dzc)
    if scale is not None and (scale.dtype != torch.float32 or not scale.is_cuda or scale.numel() != 1):
        raise ValueError("head_grad_split: scale must be one fp32 value on the device")
    _launch(lib().dy_head_grad_split, (gp, ldg, _rows(g), nb, nc, ncp, scale.data_ptr() if scale is not None else None, bp, ldb, cp, ldc, dy_dtype(dtype)),
            keep=(g, dzb, dzc, scale))
    return dzb, dzc


ANGLE_PAD = 8  # channels of the OBB angle tail's padded maps (OBB.ANGLE_COUT; kObbAngleCout in csrc/obb_loss.hip)


def obb_angle_grad_cast(g: torch.Tensor, dtype: torch.dtype, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dy_obb_angle_grad_cast``: ``g`` an fp32 NHWC view (n, >= 1, h, w) whose channel 0 is d loss / d angle logit -> (n, 8, h, w) of
    ``dtype``: g[:, 0] * scale in channel 0, zeros behind.  ``scale``: a device fp32 scalar or None."""
    n, _, h, w = g.shape
    if g.dtype != torch.float32:
        raise ValueError("obb_angle_grad_cast: g must be fp32")
    if scale is not None and (scale.dtype != torch.float32 or not scale.is_cuda or scale.numel() != 1):
        raise ValueError("obb_angle_grad_cast: scale must be one fp32 value on the device")
    gp, ldg = view_params(g[:, :1])
    dz = alloc_nhwc(n, ANGLE_PAD, h, w, dtype, g.device)
    dp, ldd = view_params(dz)
    _launch(lib().dy_obb_angle_grad_cast, (gp, ldg, n * h * w, scale.data_ptr() if scale is not None else None, dp, ldd, dy_dtype(dtype)), keep=(g, dz, scale))
    return dz


def space_to_depth2(x: torch.Tensor) -> torch.Tensor:
    """(n, c, 2h, 2w) -> (n, 4c, h, w), out[:, (a * 2 + b) * c + o, y, x] = x[:, o, 2y + a, 2x + b] (``dy_space_to_depth2_nhwc``): the inverse of
    ``depth_to_space2``, for the backward of Proto's transposed convolution."""
    require_device(x, "space_to_depth2 input")
    n, c, h2, w2 = x.shape
    if h2 % 2 or w2 % 2:
        raise ValueError("space_to_depth2: even height and width are expected")
    out = alloc_nhwc(n, 4 * c, h2 // 2, w2 // 2, x.dtype, x.device)
    (xp, lds), (op, ldd) = view_params(x), view_params(out)
    _launch(lib().dy_space_to_depth2_nhwc, (xp, op, n, h2 // 2, w2 // 2, c, lds, ldd, dy_dtype(x.dtype)), keep=(x, out))
    return out


def grad_cast_scaled(g: torch.Tensor, dtype: torch.dtype, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dy_grad_cast_scaled``: ``g`` an fp32 NHWC view (n, c, h, w), c a multiple of 8 -> the same map in ``dtype``, times ``scale`` (a device
    fp32 scalar or None): the dz of the convolution gradients from a loss kernel's fp32 gradient map."""
    n, c, h, w = g.shape
    if g.dtype != torch.float32:
        raise ValueError("grad_cast_scaled: g must be fp32")
    if scale is not None and (scale.dtype != torch.float32 or not scale.is_cuda or scale.numel() != 1):
        raise ValueError("grad_cast_scaled: scale must be one fp32 value on the device")
    gp, ldg = view_params(g)
    dz = alloc_nhwc(n, c, h, w, dtype, g.device)
    dp, ldd = view_params(dz)
    _launch(lib().dy_grad_cast_scaled, (gp, ldg, n * h * w, c, scale.data_ptr() if scale is not None else None, dp, ldd, dy_dtype(dtype)), keep=(g, dz, scale))
    return dz


def add_nhwc(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    n, c, h, w = a.shape
    if out is None:
        out = alloc_nhwc(n, c, h, w, a.dtype, a.device)
    (ap, lda), (bp, ldb), (op, ldo) = view_params(a), view_params(b), view_params(out)
    _launch(lib().dy_add_nhwc, (ap, bp, op, _rows(a), c, lda, ldb, ldo, dy_dtype(a.dtype)), keep=(a, b, out))
    return out


def sumsq_into(acc: torch.Tensor, g: torch.Tensor) -> None:
    """acc (device double scalar) += sum(g^2); g: contiguous fp32."""
    _launch(lib().dy_sumsq_f32, (g.data_ptr(), g.numel(), acc.data_ptr()), keep=(acc, g))


def sgd_step_(p: torch.Tensor, grad: torch.Tensor, buf: torch.Tensor, lr: float, momentum: float, weight_decay: float, nesterov: bool,
              first_step: bool, grad_sumsq: Optional[torch.Tensor] = None, max_norm: float = 10.0, amp_state: Optional[torch.Tensor] = None) -> None:
    _launch(lib().dy_sgd_step, (p.data_ptr(), grad.data_ptr(), buf.data_ptr(), p.numel(), lr, momentum, weight_decay, int(nesterov), int(first_step),
                                grad_sumsq.data_ptr() if grad_sumsq is not None else None, max_norm, amp_state.data_ptr() if amp_state is not None else None),
            keep=(p, grad, buf, grad_sumsq, amp_state))


def adamw_step_(p: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor, lr: float, betas, eps: float, weight_decay: float, step: int,
                grad_sumsq: Optional[torch.Tensor] = None, max_norm: float = 10.0, amp_state: Optional[torch.Tensor] = None) -> None:
    _launch(lib().dy_adamw_step, (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, betas[0], betas[1], eps, weight_decay, step,
                                  grad_sumsq.data_ptr() if grad_sumsq is not None else None, max_norm, amp_state.data_ptr() if amp_state is not None else None),
            keep=(p, grad, m, v, grad_sumsq, amp_state))


def amp_update_(amp_state: torch.Tensor, grad_sumsq: torch.Tensor, growth: float = 2.0, backoff: float = 0.5, interval: int = 2000) -> None:
    """``GradScaler.update()`` on the device state {scale, growth tracker, found_inf, skipped} (fp32[4]); no host synchronisation."""
    assert amp_state.dtype == torch.float32 and amp_state.numel() >= 4 and grad_sumsq.dtype == torch.float64
    _launch(lib().dy_amp_update, (amp_state.data_ptr(), grad_sumsq.data_ptr(), growth, backoff, interval), keep=(amp_state, grad_sumsq))


def ema_update_(ema: torch.Tensor, p: torch.Tensor, decay: float) -> None:
    _launch(lib().dy_ema_update, (ema.data_ptr(), p.data_ptr(), p.numel(), decay), keep=(ema, p))


def grad_sink_flush_(entries: torch.Tensor, grad: torch.Tensor, sink: torch.Tensor) -> None:
    """grad += sink, sink = 0 for every parameter block of ``entries`` (device int64 (n, 4): offset, cout, cin, kk) in one
    ``dy_grad_sink_flush`` launch; conv-weight blocks of ``sink`` are in the weight-gradient kernels' (cout, k, k, cin) order."""
    _launch(lib().dy_grad_sink_flush, (entries.data_ptr(), entries.shape[0], grad.data_ptr(), sink.data_ptr()), keep=(entries, grad, sink))


# ---- image sources ------------------------------------------------------------------------------------------------------


def letterbox(frames: torch.Tensor, new_w: int, new_h: int, top: int, left: int, hn: int, wn: int, swap_rb: bool = True,
              pad_value: float = 114.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 (N, H, W, 3) frames -> fp32 NCHW (N, 3, hn, wn) / 255 with the resized image at (top, left), 114 elsewhere."""
    require_device(frames, "frames")
    n, h0, w0, _ = frames.shape
    if out is None:
        out = torch.empty((n, 3, hn, wn), dtype=torch.float32, device=frames.device)
    _launch(lib().dy_letterbox_u8_to_nchw_f32, (frames.data_ptr(), out.data_ptr(), n, h0, w0, new_w, new_h, top, left, hn, wn, int(swap_rb), pad_value),
            keep=(frames, out))
    return out


def resize_bilinear_u8(img: torch.Tensor, size) -> torch.Tensor:
    """uint8 NCHW batch -> fp32 NCHW of ``size`` = interpolate(img.float() / 255, size, mode="bilinear", align_corners=False): the
    ``multi_scale`` branch of preprocess_batch (models/yolo/detect/train.py:60-73) in one kernel."""
    require_device(img, "image batch")
    if img.dtype != torch.uint8 or img.dim() != 4 or not img.is_contiguous():
        raise ValueError("resize_bilinear_u8 expects a contiguous uint8 (N, C, H, W) device tensor")
    n, c, h, w = img.shape
    ho, wo = int(size[0]), int(size[1])
    out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=img.device)
    _launch(lib().dy_resize_bilinear_u8_nchw_f32, (img.data_ptr(), out.data_ptr(), n, c, h, w, ho, wo), keep=(img, out))
    return out


def scale_img(img: torch.Tensor, ratio: float, gs: int = 32, flip_lr: bool = False) -> torch.Tensor:
    """``scale_img(img.flip(3) if flip_lr else img, ratio, gs=gs)`` of the reference (utils/torch_utils.py:436-445) in one kernel: bilinear resize to
    (int(h r), int(w r)), padded right / bottom with 0.447 to the next multiples of ``gs`` of (h r, w r) — the image pyramid of test-time augmentation."""
    import math

    require_device(img, "image batch")
    if img.dtype != torch.float32 or img.dim() != 4 or not img.is_contiguous():
        raise ValueError("scale_img expects a contiguous fp32 (N, C, H, W) device tensor")
    n, c, h, w = img.shape
    if ratio == 1.0 and not flip_lr:
        return img
    hs, ws = (int(h * ratio), int(w * ratio)) if ratio != 1.0 else (h, w)
    ho, wo = ((math.ceil(h * ratio / gs) * gs, math.ceil(w * ratio / gs) * gs) if ratio != 1.0 else (h, w))
    out = torch.empty((n, c, ho, wo), dtype=torch.float32, device=img.device)
    _launch(lib().dy_scale_img_nchw_f32, (img.data_ptr(), out.data_ptr(), n, c, h, w, hs, ws, ho, wo, int(flip_lr), 0.447), keep=(img, out))
    return out


# ---- pose: keypoint decode, keypoint rescale, batched person crops (csrc/pose.hip) ----------------------------------
CROP_COLS = 9  # columns of a crop table row: frame, x0, y0, cw, ch, new_w, new_h, top, left


def _kpt_desc(levels: Sequence[torch.Tensor], strides: Sequence[float], kpt_shape, n: int) -> "_lib.KptDecodeDesc":
    nkpt, ndim = int(kpt_shape[0]), int(kpt_shape[1])
    if len(levels) > _lib.DY_MAX_LEVELS or len(levels) != len(strides):
        raise ValueError("kpt_decode: one stride per level, at most DY_MAX_LEVELS levels")
    d = _lib.KptDecodeDesc()
    for i, t in enumerate(levels):
        require_device(t, "keypoint map")
        if t.dtype != torch.float32 or t.shape[0] != n or t.shape[1] != nkpt * ndim:
            raise ValueError(f"kpt_decode: keypoint maps must be fp32 (N, {nkpt * ndim}, h, w) NHWC views")
        d.level[i], d.ld[i] = view_params(t)
        d.h[i], d.w[i], d.stride[i] = t.shape[2], t.shape[3], float(strides[i])
    d.n_levels, d.batch, d.nkpt, d.ndim = len(levels), n, nkpt, ndim
    d.anchors = sum(t.shape[2] * t.shape[3] for t in levels)
    return d


def kpt_decode(levels: Sequence[torch.Tensor], strides: Sequence[float], kpt_shape, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Pose.kpts_decode`` of every anchor (``dy_kpt_decode``, dense form): the per-level fp32 NHWC keypoint logits (N, nk, h_i, w_i) ->
    ``pred_kpt`` (N, nk, A) fp32."""
    n = levels[0].shape[0]
    d = _kpt_desc(levels, strides, kpt_shape, n)
    shape = (n, d.nkpt * d.ndim, d.anchors)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=levels[0].device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"kpt_decode: out must be a contiguous fp32 {shape} tensor")
    d.pred_kpt = out.data_ptr()
    _launch(lib().dy_kpt_decode, (C.byref(d),), keep=(d, out, *levels))
    return out


def kpt_gather(bufs: "NmsBuffers", levels: Sequence[torch.Tensor], strides: Sequence[float], kpt_shape, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The kept rows' decoded keypoints -> (N, max_det, nk) fp32 (``dy_kpt_decode``, gather form; call it behind ``nms``).  Rows beyond the
    counts are left as they are."""
    n, md = bufs.batch, bufs.max_det
    d = _kpt_desc(levels, strides, kpt_shape, n)
    if d.anchors != bufs.anchors:
        raise ValueError(f"kpt_gather: the levels hold {d.anchors} anchors, the NMS buffers {bufs.anchors}")
    shape = (n, md, d.nkpt * d.ndim)
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=bufs.out.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"kpt_gather: out must be a contiguous fp32 {shape} tensor")
    d.counts, d.index, d.max_det, d.out = bufs.count.data_ptr(), bufs.index.data_ptr(), md, out.data_ptr()
    _launch(lib().dy_kpt_decode, (C.byref(d),), keep=(d, bufs, out, *levels))
    return out


def scale_coords_(kpts: torch.Tensor, count: torch.Tensor, params: torch.Tensor, kpt_shape, boxes: Optional[torch.Tensor] = None) -> None:
    """In-place ``ops.scale_coords`` + the ``Keypoints`` masking of the kept rows (``dy_scale_coords``).  kpts: fp32 (N, max_det, nk);
    count: int32 (N); params: device fp32 (N, 7) gain, pad_x, pad_y, clip_w, clip_h, off_x, off_y (unrounded pads); ``boxes``: the
    (N, max_det, 6) rows behind ``scale_boxes_``, whose xyxy take a non-zero offset too."""
    nkpt, ndim = int(kpt_shape[0]), int(kpt_shape[1])
    if kpts.dtype != torch.float32 or kpts.dim() != 3 or kpts.shape[2] != nkpt * ndim or not kpts.is_contiguous():
        raise ValueError(f"scale_coords_: kpts must be a contiguous fp32 (N, max_det, {nkpt * ndim}) tensor")
    n, md = kpts.shape[0], kpts.shape[1]
    if tuple(params.shape) != (n, 7) or params.dtype != torch.float32 or not params.is_contiguous() or count.dtype != torch.int32 or count.numel() != n:
        raise ValueError("scale_coords_: params must be fp32 (N, 7) and count int32 (N)")
    require_device(kpts, "keypoint rows")
    if boxes is not None and (tuple(boxes.shape) != (n, md, 6) or boxes.dtype != torch.float32 or not boxes.is_contiguous()):
        raise ValueError("scale_coords_: boxes must be the contiguous fp32 (N, max_det, 6) rows of nms")
    _launch(lib().dy_scale_coords, (kpts.data_ptr(), boxes.data_ptr() if boxes is not None else None, count.data_ptr(), params.data_ptr(), n, md, nkpt, ndim),
            keep=(kpts, boxes, count, params))


def crops_letterbox(frames: torch.Tensor, table: torch.Tensor, hn: int, wn: int, out: Optional[torch.Tensor] = None, swap_rb: bool = True,
                    pad_value: float = 114.0, table_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 (F, H, W, 3) device frames + a HOST int32 (K, 9) crop table (frame, x0, y0, cw, ch, new_w, new_h, top, left) -> fp32
    (K, 3, hn, wn) / 255, crop j letterboxed as ``letterbox`` does a contiguous copy of its window: one
    ``dy_crops_letterbox_u8_to_nchw_f32`` launch.  The table is checked on the host (a bad row raises, nothing is launched) and uploaded
    (``table_dev``: a device copy the caller already made)."""
    require_device(frames, "frames")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("crops_letterbox expects a contiguous uint8 (F, H, W, 3) device tensor")
    if table.is_cuda or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != CROP_COLS or not table.is_contiguous() or table.shape[0] < 1:
        raise ValueError("crops_letterbox expects the crop table as a contiguous int32 (K, 9) host tensor")
    f, hf, wf, _ = frames.shape
    k = int(table.shape[0])
    if out is None:
        out = torch.empty((k, 3, hn, wn), dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != (k, 3, hn, wn) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"crops_letterbox: out must be a contiguous fp32 ({k}, 3, {hn}, {wn}) tensor")
    if table_dev is None:
        table_dev = table.to(frames.device, non_blocking=True)
    _launch(lib().dy_crops_letterbox_u8_to_nchw_f32, (frames.data_ptr(), table_dev.data_ptr(), table.data_ptr(), out.data_ptr(), f, hf, wf, k, int(hn), int(wn),
                                                      int(swap_rb), float(pad_value)), keep=(frames, table, table_dev, out))
    return out


# ---- tiled inference on batches of frames (csrc/tile_merge.hip) -------------------------------------------------


def tiles_batch(frames: torch.Tensor, offsets: torch.Tensor, tile: int, out: Optional[torch.Tensor] = None, swap_rb: bool = True,
                pad_value: float = 114.0) -> torch.Tensor:
    """uint8 (F, H, W, 3) frames -> fp32 (F * K, 3, tile, tile) / 255, tile ``f * K + k`` cut at ``offsets[k] = (y, x)`` (device int32 (K, 2),
    shared by all frames), ``pad_value`` beyond the frame edge: one ``dy_tiles_batch_u8_to_nchw_f32`` launch, no host synchronisation."""
    require_device(frames, "frames")
    require_device(offsets, "tile offsets")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("tiles_batch expects a contiguous uint8 (F, H, W, 3) device tensor")
    if offsets.dtype != torch.int32 or offsets.dim() != 2 or offsets.shape[1] != 2 or not offsets.is_contiguous():
        raise ValueError("tiles_batch expects the tile offsets as a contiguous int32 (K, 2) device tensor")
    f, hf, wf, _ = frames.shape
    k, tile = int(offsets.shape[0]), int(tile)
    if out is None:
        out = torch.empty((f * k, 3, tile, tile), dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != (f * k, 3, tile, tile) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"tiles_batch: out must be a contiguous fp32 ({f * k}, 3, {tile}, {tile}) tensor")
    _launch(lib().dy_tiles_batch_u8_to_nchw_f32, (frames.data_ptr(), offsets.data_ptr(), out.data_ptr(), f, k, hf, wf, tile, tile, int(swap_rb), float(pad_value)),
            keep=(frames, offsets, out))
    return out


class TileMergeBuffers:
    """Persistent outputs + workspace of ``dy_tile_merge`` for one (frames, tiles, max_det, merge_max_det).  ``out`` / ``count`` / ``index`` /
    ``batch`` / ``max_det`` mean what they mean on ``NmsBuffers`` (``max_det`` = merge_max_det), so whatever reads NMS output reads this.
    ``fuse=True`` (or the first ``tile_merge`` call with a fusing mode) adds what ``dy_tile_fuse`` needs: ``members`` (frames, merge_max_det)
    int32 and ``fuse_workspace``; ``members`` stays ``None`` on buffers that only ever suppress."""

    ROW = 6  # x1, y1, x2, y2, conf, cls

    def __init__(self, frames: int, tiles: int, tile_max_det: int, merge_max_det: int, device, fuse: bool = False):
        self.batch, self.tiles, self.tile_max_det, self.max_det = int(frames), int(tiles), int(tile_max_det), int(merge_max_det)
        nbytes = lib().dy_tile_merge_workspace_bytes(self.batch, self.tiles, self.tile_max_det)
        if nbytes < 0:
            raise ValueError(f"tile_merge: {tiles} tiles x max_det {tile_max_det} is beyond the kernel's 32768 slots per frame")
        self.workspace = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        self.out = torch.empty((self.batch, self.max_det, self.ROW), dtype=torch.float32, device=device)
        self.count = torch.empty((self.batch,), dtype=torch.int32, device=device)
        self.index = torch.empty((self.batch, self.max_det), dtype=torch.int32, device=device)
        self.members: Optional[torch.Tensor] = None
        self.fuse_workspace: Optional[torch.Tensor] = None
        if fuse:
            self.enable_fuse()

    def enable_fuse(self) -> None:
        """Allocate (once) ``members`` and the workspace of ``dy_tile_fuse``."""
        if self.members is not None:
            return
        nbytes = lib().dy_tile_fuse_workspace_bytes(self.batch, self.tiles, self.tile_max_det, self.max_det)
        if nbytes < 0:
            raise ValueError(f"tile_merge: merge_max_det {self.max_det} is beyond the fusing kernel's 4096 rows per frame")
        self.fuse_workspace = torch.empty((nbytes,), dtype=torch.uint8, device=self.out.device)
        self.members = torch.empty((self.batch, self.max_det), dtype=torch.int32, device=self.out.device)


class RTileMergeBuffers(TileMergeBuffers):
    """``TileMergeBuffers`` of ``dy_tile_merge_rotated``: ``out`` (frames, merge_max_det, 7) = x, y, w, h, theta, conf, cls; ``out`` / ``count`` /
    ``index`` / ``batch`` / ``max_det`` mean what they mean on ``RNmsBuffers``.  The workspace is ``dy_tile_merge``'s (the sort keys)."""

    ROW = 7

    def enable_fuse(self) -> None:
        raise NotImplementedError("tile_merge_rotated: fusing merges (union / wbf) are not built for oriented boxes")


_TILE_MERGE_BUFS: dict = {}  # (buffer class, device, frames, tiles, max_det, merge_max_det) -> buffers
TILE_MERGE_METRICS = {"iou": 0, "ios": 1}
TILE_MERGE_MODES = {"suppress": 0, "union": 1, "wbf": 2}


def _tile_merge_inputs(who: str, row: int, nms_bufs, offsets: torch.Tensor, K: int):
    """The per-tile rows (``row`` floats wide) and counts of ``nms_bufs``, checked with ``offsets`` against ``K`` tiles a frame: rows, counts,
    frames, per-tile max_det."""
    rows, counts = (nms_bufs.out, nms_bufs.count) if hasattr(nms_bufs, "out") else nms_bufs
    require_device(rows, "per-tile rows")
    require_device(counts, "per-tile counts")
    require_device(offsets, "tile offsets")
    K = int(K)
    if rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[2] != row or not rows.is_contiguous() or rows.shape[0] % K or counts.dtype != torch.int32 \
            or counts.numel() != rows.shape[0] or not counts.is_contiguous():
        raise ValueError(f"{who}: rows must be contiguous fp32 (F * {K}, max_det, {row}) with as many int32 counts")
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (K, 2) or not offsets.is_contiguous():
        raise ValueError(f"{who}: offsets must be a contiguous int32 ({K}, 2) device tensor")
    return rows, counts, rows.shape[0] // K, int(rows.shape[1])


def _tile_merge_bufs(cls, bufs, device, sizes: Tuple[int, int, int, int]):
    """``bufs`` when it has ``cls``'s rows on ``device`` at ``sizes`` = (frames, tiles, max_det, merge_max_det), else the persistent ``cls``
    buffers of that device and those sizes."""
    if bufs is None or bufs.ROW != cls.ROW or (bufs.batch, bufs.tiles, bufs.tile_max_det, bufs.max_det) != sizes or bufs.out.device != device:
        key = (cls, device) + sizes
        bufs = _TILE_MERGE_BUFS.get(key)
        if bufs is None:
            bufs = _TILE_MERGE_BUFS[key] = cls(*sizes, device)
    return bufs


def _tile_merge_code(what: str, value, names: dict) -> int:
    """The code of a metric / mode given by name (any case) or by code."""
    if isinstance(value, str):
        if value.lower() not in names:
            raise ValueError(f"tile_merge: {what} '{value}', expected one of {sorted(names)}")
        return names[value.lower()]
    return int(value)


def _tile_merge_launch(fn, d, rows, counts, offsets, frame_hw, nc, thr, agnostic, bufs: TileMergeBuffers, workspace: torch.Tensor) -> TileMergeBuffers:
    """Fill what the three merge descriptors share and launch ``fn`` on ``d``."""
    d.rows, d.counts, d.offsets_yx = rows.data_ptr(), counts.data_ptr(), offsets.data_ptr()
    d.frames, d.tiles, d.max_det, d.nc = bufs.batch, bufs.tiles, bufs.tile_max_det, int(nc)
    d.frame_h, d.frame_w = int(frame_hw[0]), int(frame_hw[1])
    d.thr, d.agnostic, d.merge_max_det = float(thr), int(bool(agnostic)), bufs.max_det
    d.out, d.out_count, d.out_index = bufs.out.data_ptr(), bufs.count.data_ptr(), bufs.index.data_ptr()
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel()
    _launch(fn, (C.byref(d),), keep=(d, rows, counts, offsets, bufs))
    return bufs


def tile_merge(nms_bufs, offsets: torch.Tensor, K: int, frame_hw: Tuple[int, int], nc: int, thr: float, metric=0, agnostic: bool = False,
               merge_max_det: int = 1000, bufs: Optional[TileMergeBuffers] = None, mode="suppress") -> TileMergeBuffers:
    """Cross-tile merge of F frames in one ``dy_tile_merge`` launch; no host synchronisation.  ``nms_bufs``: the per-tile ``NmsBuffers`` of the
    (F * K)-tile batch (rows in tile pixels, clipped to the tile) or a ``(rows, counts)`` pair; ``offsets``: device int32 (K, 2) = (y, x);
    ``metric``: 0 / "iou" or 1 / "ios" (intersection over the smaller box).  ``mode``: 0 / "suppress" drops what a kept row suppresses; 1 / "union"
    and 2 / "wbf" go through one ``dy_tile_fuse`` launch instead: the same rows are kept, each with the bounding box / the score-weighted mean
    of itself and the rows it absorbed, and ``bufs.members`` counts them.  Returns rows in frame pixels, clamped to the frame, in buffers
    that persist per (F, K, max_det, merge_max_det): the next call with the same sizes overwrites them."""
    rows, counts, f, md = _tile_merge_inputs("tile_merge", 6, nms_bufs, offsets, K)
    metric = _tile_merge_code("metric", metric, TILE_MERGE_METRICS)
    mode = _tile_merge_code("mode", mode, TILE_MERGE_MODES)
    if mode not in TILE_MERGE_MODES.values():
        raise ValueError(f"tile_merge: mode {mode}, expected 0 (suppress), 1 (union) or 2 (wbf)")
    bufs = _tile_merge_bufs(TileMergeBuffers, bufs, rows.device, (f, int(K), md, int(merge_max_det)))
    if mode == 0:
        d, fn, workspace = TileMergeDesc(), lib().dy_tile_merge, bufs.workspace
    else:
        bufs.enable_fuse()
        d, fn, workspace = TileFuseDesc(), lib().dy_tile_fuse, bufs.fuse_workspace
        d.mode, d.out_members = mode, bufs.members.data_ptr()
    d.metric = metric
    return _tile_merge_launch(fn, d, rows, counts, offsets, frame_hw, nc, thr, agnostic, bufs, workspace)


def tile_merge_rotated(nms_bufs, offsets: torch.Tensor, K: int, frame_hw: Tuple[int, int], nc: int, thr: float, agnostic: bool = False,
                       merge_max_det: int = 1000, bufs: Optional[RTileMergeBuffers] = None) -> RTileMergeBuffers:
    """Cross-tile merge of F frames of oriented boxes in one ``dy_tile_merge_rotated`` launch; no host synchronisation.  ``nms_bufs``: the
    per-tile ``RNmsBuffers`` of the (F * K)-tile batch (rows x, y, w, h, theta, conf, cls in tile pixels) or a ``(rows, counts)`` pair;
    ``offsets``: device int32 (K, 2) = (y, x); ``thr``: the ProbIoU at or above which a kept row of the same class (any class with
    ``agnostic``) suppresses a candidate -- greedily, as ``tile_merge`` does.  Returns rows in frame pixels, centre and size clamped to the
    frame, in buffers that persist per (F, K, max_det, merge_max_det): the next call with the same sizes overwrites them."""
    rows, counts, f, md = _tile_merge_inputs("tile_merge_rotated", 7, nms_bufs, offsets, K)
    bufs = _tile_merge_bufs(RTileMergeBuffers, bufs, rows.device, (f, int(K), md, int(merge_max_det)))
    return _tile_merge_launch(lib().dy_tile_merge_rotated, _lib.TileMergeRotatedDesc(), rows, counts, offsets, frame_hw, nc, thr, agnostic, bufs, bufs.workspace)


# ---- frame masks of tiled segmentation (csrc/tile_merge.hip: the owner map; csrc/mask_ops.hip: the assembly) --------------------


TILE_MASK_STRIDES = (1, 2, 4)


def tile_mask_owner(nms_bufs, offsets: torch.Tensor, K: int, merged, thr: float, metric=0, agnostic: bool = False, stitch: bool = False,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Which kept frame row every per-tile candidate belongs to: int32 (F, K * max_det), one ``dy_tile_mask_owner`` launch behind the merge, no
    host synchronisation.  ``nms_bufs`` / ``offsets`` / ``K`` / ``thr`` / ``metric`` / ``agnostic``: what ``tile_merge`` was given;
    ``merged``: what it returned (or an ``(index, count)`` pair).  The slot of kept row t gets t; with ``stitch`` a candidate that is not
    kept gets the kept row that absorbs it under ``dy_tile_fuse``'s rule; every other slot -1."""
    rows, counts, f, md = _tile_merge_inputs("tile_mask_owner", 6, nms_bufs, offsets, K)
    index, count = merged if isinstance(merged, (tuple, list)) else (merged.index, merged.count)
    require_device(index, "kept index")
    require_device(count, "kept count")
    if index.dtype != torch.int32 or index.dim() != 2 or index.shape[0] != f or not index.is_contiguous() or count.dtype != torch.int32 \
            or count.numel() != f or not count.is_contiguous():
        raise ValueError(f"tile_mask_owner: the merge's index must be contiguous int32 ({f}, merge_max_det) with {f} int32 counts")
    n = int(K) * md
    if out is None:
        out = torch.empty((f, n), dtype=torch.int32, device=rows.device)
    elif tuple(out.shape) != (f, n) or out.dtype != torch.int32 or not out.is_contiguous() or out.device != rows.device:
        raise ValueError(f"tile_mask_owner: out must be a contiguous int32 ({f}, {n}) tensor on the rows' device")
    d = _lib.TileMaskOwnerDesc()
    d.rows, d.counts, d.offsets_yx, d.kept_index, d.kept_count = rows.data_ptr(), counts.data_ptr(), offsets.data_ptr(), index.data_ptr(), count.data_ptr()
    d.frames, d.tiles, d.max_det, d.merge_max_det = f, int(K), md, int(index.shape[1])
    d.thr, d.metric, d.agnostic, d.stitch = float(thr), _tile_merge_code("metric", metric, TILE_MERGE_METRICS), int(bool(agnostic)), int(bool(stitch))
    d.owner = out.data_ptr()
    _launch(lib().dy_tile_mask_owner, (C.byref(d),), keep=(d, rows, counts, offsets, index, count, out))
    return out


def tile_process_mask(protos: torch.Tensor, side: torch.Tensor, counts: torch.Tensor, offsets: torch.Tensor, owner: torch.Tensor,
                      dest: torch.Tensor, total: int, tile_hw: Tuple[int, int], frame_hw: Tuple[int, int], stride: int = 4,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The frame masks of tiled inference in one ``dy_tile_process_mask`` launch: uint8 (total, ceil(frame_h / stride), ceil(frame_w / stride)).
    ``protos``: fp32 NHWC view (F * K, 32, mh, mw) with (mh, mw) a quarter of the tile; ``side``: ``mask_gather``'s output of the tiles;
    ``counts``: the per-tile counts; ``offsets``: device int32 (K, 2) = (y, x); ``owner``: ``tile_mask_owner``'s map (F, K * max_det);
    ``dest``: int32 (F, merge_max_det), the output mask of every kept row or -1.  Mask ``dest[f, t]`` is the OR of the tile masks of the
    slots that kept row t owns, each pasted at its tile's offset; at stride 1 a tile's part is ``process_mask``'s output bit for bit."""
    for t, what in ((protos, "protos"), (side, "side"), (counts, "counts"), (offsets, "tile offsets"), (owner, "owner"), (dest, "dest")):
        require_device(t, what)
    fk, nm, mh, mw = protos.shape
    k = int(offsets.shape[0])
    if protos.dtype != torch.float32 or side.dtype != torch.float32 or not side.is_contiguous() or side.dim() != 3 or side.shape[0] != fk or side.shape[2] != 4 + nm:
        raise ValueError("tile_process_mask: protos must be fp32 (F * K, nm, mh, mw), side a contiguous fp32 (F * K, max_det, 4 + nm) tensor")
    if nm != NM:
        raise NotImplementedError(f"tile_process_mask: {nm} mask coefficients; dy_tile_process_mask is built for {NM}")
    if int(stride) not in TILE_MASK_STRIDES:
        raise ValueError(f"tile_process_mask: stride {stride}, expected one of {TILE_MASK_STRIDES}")
    md = int(side.shape[1])
    if offsets.dtype != torch.int32 or offsets.dim() != 2 or offsets.shape[1] != 2 or not offsets.is_contiguous() or k == 0 or fk % k:
        raise ValueError("tile_process_mask: offsets must be a contiguous int32 (K, 2) tensor with F * K tiles in protos")
    f = fk // k
    if counts.dtype != torch.int32 or counts.numel() != fk or not counts.is_contiguous():
        raise ValueError(f"tile_process_mask: counts must be {fk} contiguous int32")
    if owner.dtype != torch.int32 or tuple(owner.shape) != (f, k * md) or not owner.is_contiguous():
        raise ValueError(f"tile_process_mask: owner must be a contiguous int32 ({f}, {k * md}) tensor")
    if dest.dtype != torch.int32 or dest.dim() != 2 or dest.shape[0] != f or not dest.is_contiguous():
        raise ValueError(f"tile_process_mask: dest must be a contiguous int32 ({f}, merge_max_det) tensor")
    stride, total = int(stride), int(total)
    oh, ow = -(-int(frame_hw[0]) // stride), -(-int(frame_hw[1]) // stride)
    if out is None:
        out = torch.empty((total, oh, ow), dtype=torch.uint8, device=protos.device)
    elif out.dtype != torch.uint8 or out.numel() != total * oh * ow or not out.is_contiguous() or out.data_ptr() % 4 or out.device != protos.device:
        raise ValueError("tile_process_mask: out must be a contiguous, 4-byte aligned uint8 tensor of total * oh * ow elements on the prototypes' device")
    else:
        out = out.view(total, oh, ow)
    d = _lib.TileProcessMaskDesc()
    d.protos, d.ld_p = view_params(protos)
    d.side, d.counts, d.offsets_yx, d.owner, d.dest, d.out = side.data_ptr(), counts.data_ptr(), offsets.data_ptr(), owner.data_ptr(), dest.data_ptr(), out.data_ptr()
    d.frames, d.tiles, d.max_det, d.merge_max_det, d.nm, d.mh, d.mw = f, k, md, int(dest.shape[1]), nm, mh, mw
    d.tile_h, d.tile_w, d.frame_h, d.frame_w, d.stride, d.total = int(tile_hw[0]), int(tile_hw[1]), int(frame_hw[0]), int(frame_hw[1]), stride, total
    if total == 0:
        return out
    _launch(lib().dy_tile_process_mask, (C.byref(d),), keep=(d, protos, side, counts, offsets, owner, dest, out))
    return out


def augment_batch(src: torch.Tensor, table: torch.Tensor, s: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mosaic + affine / perspective warp + HSV + flips of a training batch in one ``dy_augment_u8_nchw`` launch.  src: device uint8
    (N, 3, Hs, Ws) source images (channel 0 = R); table: device uint8 (B, sizeof(dy_aug_row)) rows built by ``data.augment.DeviceAugment``;
    returns (or fills ``out``) the uint8 (B, 3, s, s) batch the image stem reads."""
    require_device(src, "augmentation sources")
    require_device(table, "augmentation table")
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[1] != 3 or not src.is_contiguous():
        raise ValueError("augment_batch expects contiguous uint8 (N, 3, Hs, Ws) sources")
    if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != C.sizeof(_lib.AugRow) or not table.is_contiguous() or table.device != src.device:
        raise ValueError(f"augment_batch: table must be a contiguous uint8 (B, {C.sizeof(_lib.AugRow)}) tensor on the sources' device")
    b, s = int(table.shape[0]), int(s)
    if out is None:
        out = torch.empty((b, 3, s, s), dtype=torch.uint8, device=src.device)
    elif tuple(out.shape) != (b, 3, s, s) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f"augment_batch: out must be a contiguous uint8 ({b}, 3, {s}, {s}) tensor on the sources' device")
    n, _, hs, ws = src.shape
    _launch(lib().dy_augment_u8_nchw, (src.data_ptr(), table.data_ptr(), out.data_ptr(), n, hs, ws, b, s), keep=(src, table, out))
    return out


# ---- fused C2f block ------------------------------------------------------------------------------------------------------


class PackedC2f:
    """Folded + packed weights of a whole C2f (n = 1) for ``dy_c2f_fused``: (w, b) pairs of cv1, m[0].cv1, m[0].cv2, cv2."""

    def __init__(self, cv1, mcv1, mcv2, cv2, shortcut: bool, dtype: torch.dtype, device, act_l2e: bool = False):
        """``act_l2e``: the four (w, b) pairs were folded for the log2(e)-scaled activation domain (biases times log2 e)."""
        (w1, b1), (wa, ba), (wb, bb), (w2, b2) = cv1, mcv1, mcv2, cv2
        self.act_l2e = bool(act_l2e)
        self.cin, self.hidden, self.cout = w1.shape[1], wa.shape[0], w2.shape[0]
        self.w1, _ = pack_frag1x1(w1, b1, dtype, device)
        self.w2, _ = pack_frag1x1(w2, b2, dtype, device)
        pa = PackedConv(wa, ba, 1, 1, 1, True, dtype, device, halo=True)
        pb = PackedConv(wb, bb, 1, 1, 1, True, dtype, device, halo=True)
        if pa.layout != _lib.DY_WLAYOUT_HALO3X3 or pb.layout != _lib.DY_WLAYOUT_HALO3X3:
            raise ValueError("PackedC2f: the Bottleneck convolutions did not pack as DY_WLAYOUT_HALO3X3")
        self.wa, self.wb = pa.w, pb.w
        self.bias = torch.cat([t.detach().float().reshape(-1).cpu() for t in (b1, ba, bb, b2)]).contiguous().to(device)
        self.shortcut, self.dtype = bool(shortcut), dtype


def c2f_fused_supported(cin: int, hidden: int, cout: int, n: int, dtype: torch.dtype, cin_lo: int = 0) -> bool:
    """``cin`` counts every input channel of cv1; ``cin_lo`` of them come through a fused 2x upsample (the folded Concat)."""
    return dtype != FP8 and bool(lib().dy_c2f_fused_supported(cin, cin_lo, hidden, cout, n, dy_dtype(dtype)))


def c2f_fused(x: torch.Tensor, pk: PackedC2f, out: Optional[torch.Tensor] = None, x_lo: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Whole C2f block in one ``dy_c2f_fused`` launch; x: NHWC view (N, c, H, W) of pk.dtype.  With ``x_lo`` (N, c_lo, H/2, W/2) the
    block input is cat(upsample2x(x_lo), x) — the Upsample + Concat in front of the neck's C2f — and pk.cin = c_lo + c."""
    require_device(x, "c2f input")
    n, c, h, w = x.shape
    c_lo = 0
    if x_lo is not None:
        require_device(x_lo, "c2f upsampled input")
        c_lo = x_lo.shape[1]
        if x_lo.shape[0] != n or (2 * x_lo.shape[2], 2 * x_lo.shape[3]) != (h, w) or x_lo.dtype != x.dtype:
            raise ValueError("c2f_fused: x_lo must be the half-resolution map of the same batch and dtype")
    if c + c_lo != pk.cin or x.dtype != pk.dtype:
        raise ValueError("c2f_fused: input channels / dtype do not match the packed block")
    if out is None:
        out = alloc_nhwc(n, pk.cout, h, w, x.dtype, x.device)
    d = C2fDesc()
    (d.x, d.ld_x), (d.y, d.ld_y) = view_params(x), view_params(out)
    if x_lo is not None:
        d.x_lo, d.ld_x_lo = view_params(x_lo)
    d.w_cv1, d.w_m_cv1, d.w_m_cv2, d.w_cv2, d.bias = pk.w1.data_ptr(), pk.wa.data_ptr(), pk.wb.data_ptr(), pk.w2.data_ptr(), pk.bias.data_ptr()
    d.batch, d.h, d.w, d.cin, d.cin_lo, d.hidden, d.cout = n, h, w, pk.cin, c_lo, pk.hidden, pk.cout
    d.shortcut, d.dtype, d.act_l2e = int(pk.shortcut), dy_dtype(x.dtype), int(pk.act_l2e)
    _launch(lib().dy_c2f_fused, (C.byref(d),), keep=(d, x, x_lo, out, pk))
    return out


# ---- tail of a hidden-64 C2f block: last Bottleneck 3x3 + closing 1x1 -----------------------------------------------------


class PackedC2fTail:
    """Folded + packed weights for ``dy_c2f_tail_fused``: (w, b) of the last Bottleneck's cv2 (3x3) and of the block's closing cv2 (1x1)."""

    def __init__(self, mcv2, cv2, n: int, shortcut: bool, dtype: torch.dtype, device, act_l2e: bool = False):
        """``act_l2e``: both (w, b) pairs were folded for the log2(e)-scaled activation domain (biases times log2 e)."""
        (w3, b3), (w1, b1) = mcv2, cv2
        self.hidden, self.cout, self.n = w3.shape[0], w1.shape[0], int(n)
        if w1.shape[1] != (2 + self.n) * self.hidden:
            raise ValueError("PackedC2fTail: cv2 must read (2 + n) * hidden channels")
        p3 = PackedConv(w3, b3, 1, 1, 1, True, dtype, device, halo=True)
        if p3.layout != _lib.DY_WLAYOUT_HALO3X3:
            raise ValueError("PackedC2fTail: the Bottleneck convolution did not pack as DY_WLAYOUT_HALO3X3")
        self.w3, self.b3 = p3.w, p3.b
        self.w1, self.b1 = pack_frag1x1(w1, b1, dtype, device)
        self.shortcut, self.dtype, self.act_l2e = bool(shortcut), dtype, bool(act_l2e)


def c2f_tail_fused_supported(hidden: int, cout: int, n: int, dtype: torch.dtype, k1: int = 3, k2: int = 3, groups: int = 1) -> bool:
    return dtype in (torch.bfloat16, torch.float16) and bool(lib().dy_c2f_tail_fused_supported(hidden, cout, n, k1, k2, groups, dy_dtype(dtype)))


def c2f_tail_fused(t: torch.Tensor, ybuf: torch.Tensor, pk: PackedC2fTail, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SiLU(conv3x3(t)) (+ the last group of ``ybuf`` with the shortcut) and the closing 1x1 over cat(ybuf, that) in one
    ``dy_c2f_tail_fused`` launch.  t: (N, hidden, H, W), the last Bottleneck's cv1 output; ybuf: (N, (1 + n) * hidden, H, W), the
    head y0 | .. | y_n of the concat buffer; out: (N, cout, H, W), possibly a channel slice of a wider buffer."""
    require_device(t, "c2f tail input")
    require_device(ybuf, "c2f tail concat buffer")
    n, c, h, w = t.shape
    if t.dtype != pk.dtype or ybuf.dtype != pk.dtype or c != pk.hidden or tuple(ybuf.shape) != (n, (1 + pk.n) * pk.hidden, h, w):
        raise ValueError("c2f_tail_fused: inputs do not match the packed block")
    if out is None:
        out = alloc_nhwc(n, pk.cout, h, w, t.dtype, t.device)
    elif tuple(out.shape) != (n, pk.cout, h, w) or out.dtype != t.dtype:
        raise ValueError("c2f_tail_fused: out must be a (N, cout, H, W) view of the inputs' dtype")
    d = C2fTailDesc()
    (d.t, d.ld_t), (d.buf, d.ld_buf), (d.y, d.ld_y) = view_params(t), view_params(ybuf), view_params(out)
    d.w3, d.b3, d.w1, d.b1 = pk.w3.data_ptr(), pk.b3.data_ptr(), pk.w1.data_ptr(), pk.b1.data_ptr()
    d.batch, d.h, d.w, d.hidden, d.cout, d.n_bottlenecks = n, h, w, pk.hidden, pk.cout, pk.n
    d.shortcut, d.dtype, d.act_l2e = int(pk.shortcut), dy_dtype(t.dtype), int(pk.act_l2e)
    _launch(lib().dy_c2f_tail_fused, (C.byref(d),), keep=(d, t, ybuf, out, pk))
    return out


# ---- front of a hidden-64 C2f block: the stride-2 3x3 in front of it + the opening 1x1 ------------------------------------


class PackedC2fFront:
    """Folded + packed weights for ``dy_c2f_front_fused``: (w, b) of the stride-2 3x3 in front of the block and of the block's cv1 (1x1)."""

    def __init__(self, conv3, cv1, act: int, dtype: torch.dtype, device):
        """``act``: the activation code both convolutions were folded for (``domain_fold``): DY_ACT_SILU or DY_ACT_SILU_L2E."""
        (w3, b3), (w1, b1) = conv3, cv1
        self.cin, self.cmid, self.cout = w3.shape[1], w3.shape[0], w1.shape[0]
        self.c_other = w1.shape[1] - self.cmid
        if self.c_other < 0 or tuple(w3.shape[2:]) != (3, 3):
            raise ValueError("PackedC2fFront: cv1 must read the 3x3's output first (+ the other Concat source)")
        p3 = PackedConv(w3, b3, 2, 1, 1, act, dtype, device, halo=True)
        if p3.layout != _lib.DY_WLAYOUT_HALO3X3:
            raise ValueError("PackedC2fFront: the stride-2 convolution did not pack as DY_WLAYOUT_HALO3X3")
        self.w3, self.b3 = p3.w, p3.b
        self.w1, self.b1 = pack_frag1x1(w1, b1, dtype, device)
        self.act, self.dtype = int(act), dtype


def c2f_front_fused_supported(cin: int, cmid: int, c_other: int, cout: int, dtype: torch.dtype, act: int = DY_ACT_SILU, k: int = 3, stride: int = 2, groups: int = 1) -> bool:
    return dtype in (torch.bfloat16, torch.float16) and bool(lib().dy_c2f_front_fused_supported(cin, cmid, c_other, cout, k, stride, groups, int(act), dy_dtype(dtype)))


def c2f_front_fused(x: torch.Tensor, pk: PackedC2fFront, other: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SiLU(conv3x3 stride 2 (x)) and the C2f's opening 1x1 over cat(that, other) in one ``dy_c2f_front_fused`` launch.  x: (N, cin, H, W);
    other: (N, c_other, Ho, Wo), the second source of the Concat in front of the block (None without one); out: (N, cout, Ho, Wo), possibly
    a channel slice of a wider buffer."""
    require_device(x, "c2f front input")
    n, c, h, w = x.shape
    ho, wo = conv_out_hw(h, w, 3, 2, 1)
    if x.dtype != pk.dtype or c != pk.cin or (other is None) != (pk.c_other == 0):
        raise ValueError("c2f_front_fused: inputs do not match the packed pair")
    if other is not None:
        require_device(other, "c2f front second source")
        if tuple(other.shape) != (n, pk.c_other, ho, wo) or other.dtype != pk.dtype:
            raise ValueError("c2f_front_fused: other must be a (N, c_other, Ho, Wo) view of the input's dtype")
    if out is None:
        out = alloc_nhwc(n, pk.cout, ho, wo, x.dtype, x.device)
    elif tuple(out.shape) != (n, pk.cout, ho, wo) or out.dtype != x.dtype:
        raise ValueError("c2f_front_fused: out must be a (N, cout, Ho, Wo) view of the input's dtype")
    d = C2fFrontDesc()
    (d.x, d.ld_x), (d.y, d.ld_y) = view_params(x), view_params(out)
    if other is not None:
        d.other, d.ld_other = view_params(other)
    d.w3, d.b3, d.w1, d.b1 = pk.w3.data_ptr(), pk.b3.data_ptr(), pk.w1.data_ptr(), pk.b1.data_ptr()
    d.batch, d.h, d.w, d.cin, d.cmid, d.c_other, d.cout = n, h, w, pk.cin, pk.cmid, pk.c_other, pk.cout
    d.act, d.dtype = pk.act, dy_dtype(x.dtype)
    _launch(lib().dy_c2f_front_fused, (C.byref(d),), keep=(d, x, other, out, pk))
    return out
