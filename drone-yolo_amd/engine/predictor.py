"""Inference loop of the detection path on the device.

Reference: ``BasePredictor`` (ultralytics/engine/predictor.py:118-323: preprocess, inference,
stream_inference, setup_model) and ``DetectionPredictor`` (models/yolo/detect/predict.py:23-73:
postprocess = NMS + scale_boxes + Results).  MI355X-first differences:

* one pass = input layout/dtype conversion -> 80-odd conv launches -> decode -> NMS -> box rescale,
  all libdyolo kernels on one HIP stream, recorded once per input shape as a ``LaunchPlan`` and
  replayed (optionally from a hipGraph) afterwards — no per-image Python loop, no host syncs
  inside the pass (the reference syncs at every boolean index of ops.py:266-330).
* results stay on the device as padded (N, max_det, 6) + counts; ``Results`` are materialised with
  one device->host transfer of the counts.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Tuple

import torch

from .. import hip_ops as H
from ..utils import LOGGER, ops
from ..utils.torch_utils import select_device
from ..nn.autobackend import AutoBackend
from .results import Results

_DTYPE_NAMES = {"f16x2": H.F16X2, "split": H.F16X2, "fp8": H.FP8, "float8_e4m3fn": H.FP8, "bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp16": torch.float16, "half": torch.float16,
                "float16": torch.float16, "fp32": torch.float32, "float32": torch.float32}


# The precision a predictor runs in when the caller names none.  The reference's default is ``half: False`` = fp32 (cfg/default.yaml:54,
# engine/predictor.py:315-322), and the drop-in's default must reproduce ITS detections: class / index exact, IoU >= 0.999 (BASELINE.json).
# ``half=True`` selects float16 storage as in the reference; bf16 and fp8 only on request (they do not meet that bar).
# Two precisions meet it: fp32 storage on the fp32 MFMA (1/16 of the 16-bit rate) and split float16 (hip_ops.F16X2: every value a float16
# pair hi + lo 2^-11, three 16-bit MFMAs per product — kept sets identical to the reference's on every fixture, at ~2x the fp32 path's
# throughput).  The default is the split type wherever its kernels cover the model (dense convolutions on whole groups of 8 channels),
# fp32 otherwise (the DWConv of the -sf YAML).
EXACT_DTYPE = H.F16X2


def split_supported(model) -> bool:
    """Whether every convolution of ``model`` is one the split-float16 kernels take (dense, channel counts in whole groups of 8 — the image
    layer's input and the class logits excepted)."""
    import torch.nn as nn

    from ..nn.modules.head import Pose

    convs = [m for k, m in model.named_modules() if isinstance(m, nn.Conv2d) and ".dfl" not in k]  # (DFL's fixed 16 -> 1 conv lives inside the decode kernel)
    # a Pose head's keypoint branch (51 channels for the n, s and m scales) runs on packs padded to a served width (Pose.served_width): its channel counts are not the kernels'
    padded = {id(c) for m in model.modules() if isinstance(m, Pose) for c in m.cv4.modules() if isinstance(c, nn.Conv2d)}
    for c in convs:
        if id(c) in padded and c.groups == 1 and c.kernel_size in ((1, 1), (3, 3)) and c.stride[0] == 1:
            continue
        if c.groups != 1:  # DWConv of the -sf YAML: the small-group kernel (one output channel per group, 1 / 2 / 4 inputs each)
            if c.out_channels != c.groups or c.in_channels // c.groups not in (1, 2, 4) or c.out_channels % 8 or c.kernel_size[0] ** 2 * (c.in_channels // c.groups) * c.out_channels * 4 > 48 * 1024:
                return False
            continue
        if c.kernel_size not in ((1, 1), (3, 3)) or c.stride[0] not in (1, 2):
            return False
        if (c.in_channels % 8 and c.in_channels > 3) or (c.out_channels % 8 and c.bias is None):  # (plain biased 1x1 = Detect's fp32 outputs)
            return False
        if c.kernel_size == (3, 3) and c.in_channels > 680:  # the 3x3 tap table of csrc/conv_gemm_fk.hip (1,536 words)
            return False
    return bool(convs)


def resolve_dtype(dtype=None, half: bool = False, model=None) -> torch.dtype:
    if isinstance(dtype, torch.dtype):
        return dtype
    if dtype is None:
        if half:
            return torch.float16
        return EXACT_DTYPE if (model is None or split_supported(model)) else torch.float32
    try:
        return _DTYPE_NAMES[str(dtype).lower()]
    except KeyError:
        raise ValueError(f"unknown dtype '{dtype}', expected one of {sorted(_DTYPE_NAMES)}") from None


class CompiledForward:
    """A recorded forward for one (batch, H, W): its launch plan, static buffers and optional hipGraph."""

    def __init__(self):
        self.plan = H.LaunchPlan()
        self.pred: Optional[torch.Tensor] = None  # decoded (N, 4+nc, A) fp32
        self.nms: Optional[H.NmsBuffers] = None
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.graph_tail: Optional[torch.cuda.CUDAGraph] = None  # every launch but the first (the one that reads the image): see DetectionPredictor._capture
        self.static_in: Optional[torch.Tensor] = None
        self.weights_sig = None  # BaseModel.weights_signature() of the weights this plan baked in


class DetectionPredictor:
    """Device-resident predictor (reference predictor.py:64-323, detect/predict.py:8-73)."""

    keeps_track_index = False  # the segmentation task: ``last_track_index``, the detection every result row came from (its mask follows it)
    max_compiled = 8  # recorded (batch, H, W) passes kept alive (each holds activations, NMS buffers and a graph: a video's ragged last batch must not pile up)

    def __init__(self, model, overrides: Optional[dict] = None):
        a = dict(conf=0.25, iou=0.7, max_det=300, classes=None, agnostic_nms=False, half=False, dtype=None, device="",
                 verbose=False, graph=True, max_nms=30000, max_wh=7680, imgsz=640, fp8_layers=None, batch=None, augment=False,
                 tracker="bytetrack.yaml", device_track=True, track_streams=1, max_tracks=512,
                 tile=None, tile_overlap=0.2, merge_iou=0.7, merge_metric="iou", merge_mode="suppress", merge_max_det=1000, retina_masks=False,
                 tile_mask_stride=4, crop_expand=0.2)
        a.update(overrides or {})
        self.args = a
        if a["tile"] is not None:  # tiled inference: checked before anything touches the device
            s = int(max(model.stride)) if hasattr(model, "stride") else 32
            if int(a["tile"]) <= 0 or int(a["tile"]) % s:
                raise ValueError(f"tile = {a['tile']} must be a positive multiple of the model's largest stride {s}")
            if str(a["merge_metric"]).lower() not in H.TILE_MERGE_METRICS:
                raise ValueError(f"merge_metric = '{a['merge_metric']}', expected one of {sorted(H.TILE_MERGE_METRICS)}")
            if str(a["merge_mode"]).lower() not in H.TILE_MERGE_MODES:
                raise ValueError(f"merge_mode = '{a['merge_mode']}', expected one of {sorted(H.TILE_MERGE_MODES)}")
            if a["augment"]:
                raise NotImplementedError("augment=True with tile: the image pyramid of test-time augmentation is not built for tiles")
            if not 0.0 <= float(a["tile_overlap"]) < 1.0 or not 0.0 <= float(a["merge_iou"]) <= 1.0 or int(a["merge_max_det"]) < 1:
                raise ValueError("tile_overlap must be in [0, 1), merge_iou in [0, 1] and merge_max_det positive")
        self.tracker = None  # mode="track" (Model.track): a trackers.DeviceByteTracker / ByteTracker fed behind the NMS and box scaling of every batch
        self.device = select_device(a["device"])
        # dtype="fp8-mixed" (BASELINE config 5): float16 storage with the internals of the C2f blocks the error budget allows in
        # e4m3 (BaseModel.fp8_plan_off_p2, or the blocks given as overrides["fp8_layers"]); dtype="fp8": the whole trunk in e4m3, Detect tail float16
        self.mixed8 = isinstance(a["dtype"], str) and a["dtype"].lower().replace("_", "-") == "fp8-mixed"
        self.dtype = torch.float16 if self.mixed8 else resolve_dtype(a["dtype"], a["half"], model)
        # setup_model (predictor.py:300-323): AutoBackend moves the graph to the device, fuses, picks the precision and freezes it
        self.backend = AutoBackend(model, device=self.device, fp16=bool(a["half"]), dtype=self.dtype, fuse=False, verbose=bool(a["verbose"]))
        self.model = self.backend.model
        self._compiled: Dict[Tuple, CompiledForward] = {}
        self._tile_state: Dict[Tuple, tuple] = {}  # tile mode, per (frames, H, W): device tile offsets, the tile batch, the merge buffers
        self._classes_mask = None
        if a["classes"] is not None:
            m = torch.zeros(self.model.yaml["nc"], dtype=torch.uint8)
            m[torch.as_tensor(list(a["classes"]), dtype=torch.long)] = 1
            self._classes_mask = m.to(self.device)

    # ---- stages (names follow the reference) -------------------------------------------------------
    def preprocess(self, im) -> torch.Tensor:
        """Tensor source: BCHW float in [0,1], moved to the device (predictor.py:118-136; tensors are not /255).
        Array source — a list of HWC BGR uint8 numpy frames of ONE shape, or a uint8 (N, H, W, 3) tensor: LetterBox
        (``auto`` = minimum rectangle, as pre_transform picks for same-shape batches, predictor.py:147-163), BGR->RGB,
        HWC->CHW and /255 in one kernel; ``self.letterbox_info`` then holds what postprocess needs to map boxes back."""
        self.letterbox_info = None
        if isinstance(im, (list, tuple)) or (isinstance(im, torch.Tensor) and im.dtype == torch.uint8 and im.dim() == 4 and im.shape[-1] == 3) \
                or type(im).__name__ == "ndarray":
            import numpy as np

            from ..data.augment import LetterBox

            if not isinstance(im, torch.Tensor):
                frames = [im] if type(im).__name__ == "ndarray" and im.ndim == 3 else list(im)
                if len({f.shape for f in frames}) != 1:
                    # sources of different shapes (pre_transform, predictor.py:147-163: same_shapes False -> auto False): every image is
                    # letterboxed on its own to the full imgsz x imgsz and the batch stacked; boxes map back per image (r05)
                    lb = LetterBox(self.args.get("imgsz", 640), auto=False, stride=int(self.model.stride.max()))
                    size = lb.new_shape
                    out = torch.empty((len(frames), 3, size[0], size[1]), dtype=torch.float32, device=self.device)
                    info = []
                    for i, f in enumerate(frames):
                        if f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
                            raise ValueError("image sources must be uint8 HWC BGR frames")
                        lb.into(torch.from_numpy(np.ascontiguousarray(f)).to(self.device), out[i : i + 1], swap_rb=True)
                        info.append((f.shape[0], f.shape[1], size[0], size[1]))
                    self.letterbox_info = info
                    return out
                im = torch.from_numpy(np.ascontiguousarray(np.stack(frames)))
            frames = im.to(self.device).contiguous()
            lb = LetterBox(self.args.get("imgsz", 640), auto=True, stride=int(self.model.stride.max()))
            out = lb(frames, swap_rb=True)
            n, h0, w0, _ = frames.shape
            self.letterbox_info = (h0, w0, out.shape[2], out.shape[3])
            return out
        if not isinstance(im, torch.Tensor):
            raise NotImplementedError("sources: a float BCHW tensor in [0,1], or uint8 HWC BGR frames (list of numpy arrays / uint8 NHWC tensor)")
        if im.dim() == 3:
            im = im[None]
        if im.shape[1] != self.model.yaml.get("ch", 3):
            raise ValueError(f"expected {self.model.yaml.get('ch', 3)} input channels, got {im.shape[1]}")
        s = int(self.model.stride.max())
        if im.shape[2] % s or im.shape[3] % s:
            raise ValueError(f"tensor source must have H, W divisible by the model stride {s} (loaders.py:516-584)")
        return im.to(self.device, torch.float32, non_blocking=True).contiguous()

    def _calibrate_fp8(self, im: torch.Tensor) -> None:
        """fp8 storage (BASELINE config 5): one fp16 pass over this batch measures the largest activation the network stores;
        the network-wide activation scale puts it at 224 = half of e4m3's 448 (headroom for other inputs; e4m3 is a floating
        format, so smaller activations keep their 3-bit mantissa down to 2^-9 of the scale).  Weight scales are per output
        channel and need no data (hip_ops.PackedConv)."""
        with H.observe_absmax() as log:
            self.model._predict_once(im, image_dtype=torch.float16)
        amax = float(torch.stack(log).max()) if log else 1.0
        H.set_fp8_act_scale(max(amax / 224.0, 1e-8))
        self.fp8_calibration = {"absmax": amax, "act_scale": H.fp8_act_scale()}

    def _record(self, im: torch.Tensor) -> CompiledForward:
        cf = CompiledForward()
        a = self.args
        if self.dtype == H.FP8 or self.mixed8:
            self._calibrate_fp8(im)
        plan8 = None
        if self.mixed8:
            plan8 = frozenset(a["fp8_layers"]) if a.get("fp8_layers") is not None else self.model.fp8_plan_off_p2()
            self.fp8_calibration["fp8_layers"] = sorted(plan8)
        n, _, h, w = im.shape
        params = torch.tensor(self._box_params(h, w, n), dtype=torch.float32, device=self.device)
        cf.box_params, cf.box_key = params, self._box_params(h, w, n)
        det = self.model.model[-1]
        holder = {}

        def make_bufs(nb, anchors):  # Detect asks for the NMS buffers so that decode can fill the candidate list
            holder["bufs"] = self._new_nms_bufs(nb, anchors)
            return holder["bufs"]

        det.fused_nms = (make_bufs, float(a["conf"]), self._classes_mask)
        det.fuse_tail = True  # branch tails + decode + filter in one launch where the shape is built
        self.model.fp8_layers = plan8
        try:
            with H.record(cf.plan):
                y, aux = self.model._predict_once(im, image_dtype=self.dtype)
                cf.pred = y
                cf.nms = self._record_nms(y, aux, holder.get("bufs"))
                self._record_masks(cf, aux)  # (a segmentation model: the coefficient gather, in front of the box rescale)
                # construct_result: scale_boxes(img.shape[2:], boxes, orig.shape) — tensor sources are their own
                # original image, so gain 1 / pad 0 and the clip to (h, w) remain (detect/predict.py:59-73)
                self._record_scale(cf, params)
        finally:
            det.fused_nms = None
            det.fuse_tail = False
            self.model.fp8_layers = None
        cf.plan.keep.append(params)
        return cf

    # ---- what a task changes in the recorded pass and in its results; the detection and segmentation tasks keep the four below as they are ----
    def _new_nms_bufs(self, nb: int, anchors: int):
        """The NMS buffers the Detect kernels' candidate filter fills and the NMS of ``_record_nms`` reads."""
        return H.NmsBuffers(nb, anchors, int(self.args["max_det"]), self.device)

    def _record_nms(self, y, aux, bufs):
        """The NMS launch of the recorded pass; ``bufs``: what ``_new_nms_bufs`` made when the head's kernels filtered the candidates."""
        a = self.args
        return H.nms(y, float(a["conf"]), float(a["iou"]), max_det=int(a["max_det"]), max_nms=int(a["max_nms"]),
                     max_wh=float(a["max_wh"]), agnostic=bool(a["agnostic_nms"]), nc=self.model.yaml["nc"],
                     classes_mask=self._classes_mask, bufs=bufs, prefiltered=bufs is not None)

    def _record_scale(self, cf: CompiledForward, params: torch.Tensor) -> None:
        """construct_result's rescale of the kept rows to the original image, on the device."""
        H.scale_boxes_(cf.nms, params)

    def _result(self, img, path, names, rows, orig_shape, masks) -> Results:
        return Results(img, path, names, boxes=rows, orig_shape=orig_shape, masks=masks)

    def _record_masks(self, cf: CompiledForward, aux) -> None:
        """Hook between the NMS and the box rescale of the recorded pass; the detection task launches nothing here."""

    def _mask_stash(self, cf: CompiledForward, streamed: bool):
        """What the masks of this batch are assembled from once its counts are on the host (None: a detection model)."""
        return None

    def _masks_for(self, stash, counts, rows, im, info) -> list:
        """Per image the (k, H, W) masks of its k detections, or None."""
        return [None] * len(counts)

    def _box_params(self, h: int, w: int, n: int):
        """Per image (gain, pad_x, pad_y, clip_w, clip_h) of ops.scale_boxes (utils/ops.py:92-127) for the current source: n rows."""
        info = getattr(self, "letterbox_info", None)
        if info is None:
            return [[1.0, 0.0, 0.0, float(w), float(h)]] * n
        rows = []
        for h0, w0, hn, wn in (info if isinstance(info, list) else [info] * n):
            gain = min(hn / h0, wn / w0)
            rows.append([gain, float(round((wn - w0 * gain) / 2 - 0.1)), float(round((hn - h0 * gain) / 2 - 0.1)), float(w0), float(h0)])
        return rows

    def _forward_augment(self, im: torch.Tensor) -> CompiledForward:
        """``augment=True`` (reference predictor.py:306: ``self.model(im, augment=...)`` -> DetectionModel._predict_augment): three passes of the path over
        the image pyramid, merged along the anchors, then the NMS over the merged candidates.  Launched as it comes — nothing recorded or replayed."""
        a = self.args
        if self.dtype == H.FP8 or self.mixed8:
            raise NotImplementedError("augment=True is built for the 16-bit, split-float16 and fp32 storage types")
        cf = CompiledForward()
        y, _ = self.model._predict_augment(im, image_dtype=self.dtype)
        cf.pred = y
        cf.nms = H.nms(y, float(a["conf"]), float(a["iou"]), max_det=int(a["max_det"]), max_nms=int(a["max_nms"]), max_wh=float(a["max_wh"]),
                       agnostic=bool(a["agnostic_nms"]), nc=self.model.yaml["nc"], classes_mask=self._classes_mask)
        n, _, h, w = im.shape
        params = torch.tensor(self._box_params(h, w, n), dtype=torch.float32, device=self.device)
        H.scale_boxes_(cf.nms, params)
        cf.box_params = params
        return cf

    def forward_device(self, im: torch.Tensor) -> CompiledForward:
        """Run one batch; outputs stay on the device in the returned object's ``nms`` buffers."""
        if self.args.get("augment"):
            return self._forward_augment(im)
        key = (tuple(im.shape), self.dtype)
        cf = self._compiled.get(key)
        sig = self.model.weights_signature()
        if cf is not None and cf.weights_sig != sig:
            # the recorded plan (and its hipGraph) holds device pointers to the weight packs as they were at record time;
            # the reference predictor always runs the live model, so re-record after load_state_dict / training / .to()
            self._compiled.pop(key)
            cf = None
        if cf is not None:  # the recorded dy_scale_boxes launch reads this device tensor: refresh it when the source geometry changed
            bp = self._box_params(im.shape[2], im.shape[3], im.shape[0])
            if bp != cf.box_key:
                cf.box_params.copy_(torch.tensor(bp, dtype=torch.float32))
                cf.box_key = bp
        if cf is None:
            while len(self._compiled) >= self.max_compiled:  # a recorded pass owns its buffers and its hipGraph: keep the most recent shapes only
                self._compiled.pop(next(iter(self._compiled)))
            cf = self._compiled[key] = self._record(im)  # recording also executes the launches
            cf.weights_sig = self.model.weights_signature()  # after recording: packing may itself touch caches
            if self.args["graph"]:
                self._capture(cf, im)
            return cf
        if cf.graph is not None:
            if im.data_ptr() == cf.static_in.data_ptr():
                cf.graph.replay()
            elif cf.graph_tail is not None:
                # the caller's own tensor: the launch that reads the image runs from ITS address, the rest is the second graph — no copy of the
                # batch into the graph's static input first (fp32 640 x 640 x 256: 1.26 GB read + written, ~0.6 ms per call)
                cf.plan.rebind_input(im.data_ptr())
                cf.plan.replay(torch.cuda.current_stream().cuda_stream, 0, 1)
                cf.graph_tail.replay()
            else:
                cf.static_in.copy_(im, non_blocking=True)
                cf.graph.replay()
        else:
            cf.plan.rebind_input(im.data_ptr())
            cf.plan.replay(torch.cuda.current_stream().cuda_stream)
        return cf

    def _capture(self, cf: CompiledForward, im: torch.Tensor) -> None:
        """Capture the recorded launches into a hipGraph (replay cost ~10 us instead of ~100 launches)."""
        cf.static_in = im.clone()
        cf.plan.rebind_input(cf.static_in.data_ptr())
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        # thread_local: HIP calls of OTHER host threads (e.g. RCCL's watchdog in a torch.distributed run) must not
        # invalidate this capture
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            cf.plan.replay(torch.cuda.current_stream().cuda_stream)
        cf.graph = g
        # A second graph without the plan's first launch when that launch is the one reading the image (the fused stem / the layout cast):
        # ``forward_device`` then serves a tensor at ANY address without copying it into ``static_in`` — one eager launch + this graph.
        if cf.plan.input_slot is not None and cf.plan.input_slot[0] == 0 and len(cf.plan.ops) > 1:
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, capture_error_mode="thread_local"):
                cf.plan.replay(torch.cuda.current_stream().cuda_stream, 1)
            cf.graph_tail = g2

    def profile_layers(self, im: torch.Tensor, iters: int = 3) -> List[dict]:
        """Per-layer device time of the recorded pass for ``im``'s shape — the reference's ``_profile_one_layer`` (nn/tasks.py:171-191: time per layer
        of ``_predict_once(profile=True)``), measured the way this path runs: the plan's launches replayed one by one with HIP events on the
        launch stream and summed by the model layer that issued them (layers folded into a consumer's gather — Upsample, Concat — launch nothing
        and do not appear; NMS and the box rescale come last as 'postprocess').  Returns [{layer, type, launches, ms, kernels}]."""
        cf = self.forward_device(im)
        L, stream = H.lib(), torch.cuda.current_stream().cuda_stream
        tot, names = {}, {}
        for _ in range(iters):
            evs = []
            for i, (fn, args, _) in enumerate(cf.plan.ops):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn(*args, stream)
                e.record()
                evs.append((i, s, e))
                names[i] = (L.dy_last_kernel_name() or b"").decode() or fn.__name__
            torch.cuda.synchronize(self.device)
            for i, s, e in evs:
                tot[i] = tot.get(i, 0.0) + s.elapsed_time(e)
        rows: Dict = {}
        for i in range(len(cf.plan.ops)):
            tag = cf.plan.tags[i] if i < len(cf.plan.tags) and cf.plan.tags[i] is not None else (10 ** 6, "postprocess (NMS, box rescale; an input layout cast where layer 0 has no fused image kernel)")
            r = rows.setdefault(tag, {"layer": tag[0] if tag[0] < 10 ** 6 else None, "type": tag[1], "launches": 0, "ms": 0.0, "kernels": []})
            r["launches"] += 1
            r["ms"] += tot[i] / iters
            if names[i] not in r["kernels"]:
                r["kernels"].append(names[i])
        return [dict(r, ms=round(r["ms"], 4)) for _, r in sorted(rows.items(), key=lambda kv: kv[0][0])]

    def static_input(self, shape) -> Optional[torch.Tensor]:
        cf = self._compiled.get((tuple(shape), self.dtype))
        return None if cf is None else cf.static_in

    rotated_rows = False  # the rows behind the NMS are [x1, y1, x2, y2, conf, cls]; the oriented-box task: [x, y, w, h, r, conf, cls]

    def make_tracker(self):
        """The tracker of ``mode="track"`` for this predictor's arguments: ``device_track`` picks the kernel or the host path."""
        from ..trackers import ByteTracker, DeviceByteTracker

        a = self.args
        cls = DeviceByteTracker if a["device_track"] else ByteTracker
        max_det = int(a["max_det"])
        if a["tile"] is not None:  # the tracker reads the merged rows of a frame
            max_det = int(a["merge_max_det"])
            if max_det > 1024:
                raise ValueError(f"merge_max_det = {max_det} with mode='track': the track step takes at most 1024 detections per frame")
        return cls(a["tracker"], frame_rate=30, max_tracks=int(a["max_tracks"]), streams=int(a["track_streams"]), max_det=max_det, device=self.device,
                   rotated=self.rotated_rows)

    def _track_launch(self, cf: CompiledForward):
        """Device tracker: the track step behind this batch's NMS and box scaling, on the same stream; returns copies (rows, counts) that
        outlive the next batch.  Host tracker: None (it runs where the rows reach the host)."""
        if self.tracker is None or not hasattr(self.tracker, "bufs"):
            return None
        out, cnt = self.tracker.update_batch(cf.nms.out, cf.nms.count)
        return out.clone(), cnt

    def _boxes_of(self, i: int, k: int, rows: torch.Tensor, tracked) -> torch.Tensor:
        """The rows of image i's ``Results``: its k detections, or — when the tracker returned rows for it — those tracks
        [x1, y1, x2, y2, id, conf, cls] ([x, y, w, h, r, id, conf, cls] of an oriented-box model): the tracker's rows without their trailing
        idx column (trackers/track.py:79-88: an image without detections or without returned tracks keeps its plain result)."""
        if self.tracker is None or k == 0:
            return rows[i, :k]
        if tracked is None:  # host tracker, images in order
            t = torch.from_numpy(self.tracker.update(rows[i, :k].cpu().numpy(), stream=i % self.tracker.streams)).to(rows.device)
        else:
            t = tracked[0][i, : tracked[1][i]]
        if len(t) and self.keeps_track_index:
            self.last_track_index[i] = t[:, -1].long()
        return t[:, :-1] if len(t) else rows[i, :k]

    def _all_boxes(self, counts, rows, tracked) -> list:
        """``_boxes_of`` for every image of a batch, in order; ``last_track_index[i]`` then holds, per row of image i's result, the index of
        its detection among the image's plain rows (the tracker's idx column; 0 .. k - 1 where the plain result stands)."""
        if self.keeps_track_index:  # (a detection model needs no index: nothing is launched for it here)
            self.last_track_index = [torch.arange(k, device=rows.device) for k in counts]
        return [self._boxes_of(i, k, rows, tracked) for i, k in enumerate(counts)]

    def postprocess(self, cf: CompiledForward, im: torch.Tensor, paths=None) -> List[Results]:
        n = cf.nms.count.shape[0]
        if self.tracker is not None and n % self.tracker.streams:
            raise ValueError(f"a batch of {n} images is no multiple of track_streams = {self.tracker.streams}")
        tracked = self._track_launch(cf)
        # the pass's only device->host synchronisation: the NMS counts, with the tracker's counts behind them in the same copy
        both = (torch.cat([cf.nms.count, tracked[1]]) if tracked is not None else cf.nms.count).tolist()
        counts = both[:n]
        if tracked is not None:
            tracked = (tracked[0], both[n:])
        names = self.model.names
        out = []
        info = getattr(self, "letterbox_info", None)
        rows = cf.nms.out.clone()  # ONE copy of the padded (N, max_det, 6) rows: the next pass overwrites the buffer, the Results keep views of this one
        boxes = self._all_boxes(counts, rows, tracked)
        masks = self._masks_for(self._mask_stash(cf, streamed=False), counts, rows, im, info)
        for i, k in enumerate(counts):
            one = (info[i] if isinstance(info, list) else info) if info else None
            out.append(self._result(im[i], paths[i] if paths else f"image{i}.jpg", names, boxes[i],
                                    (one[0], one[1]) if one else im.shape[2:], masks[i]))
        return out

    # ---- image files and PIL images as sources (reference data/build.py:160-200 check_source / load_inference_source, data/loaders.py:284-420
    # LoadImagesAndVideos, :451-500 LoadPilAndNumpy).  Decoding is host glue in front of the path: PIL here (cv2 is not in the image), so a lossless
    # file (png, bmp, tif) gives the reference's pixels and a jpeg whatever PIL's libjpeg decodes; videos, streams and URLs are not built. ----------
    IMG_FORMATS = {"bmp", "jpeg", "jpg", "mpo", "png", "tif", "tiff", "webp"}

    @classmethod
    def list_image_files(cls, source) -> List[str]:
        """A file, a directory (its `*.*`, sorted), a glob pattern, a `.txt` list of such, or a list of them -> the image files, in the reference's order."""
        import glob
        import os
        from pathlib import Path

        parent = None
        if isinstance(source, (str, Path)) and Path(str(source)).suffix == ".txt":
            parent = Path(str(source)).parent
            source = Path(str(source)).read_text().splitlines()
        files = []
        for q in (sorted(str(v) for v in source) if isinstance(source, (list, tuple)) else [str(source)]):
            a = str(Path(q).absolute())
            if "*" in a:
                files.extend(sorted(glob.glob(a, recursive=True)))
            elif os.path.isdir(a):
                files.extend(sorted(glob.glob(os.path.join(a, "*.*"))))
            elif os.path.isfile(a):
                files.append(a)
            elif parent is not None and (parent / q).is_file():
                files.append(str((parent / q).absolute()))
            else:
                raise FileNotFoundError(f"{q} does not exist")
        images = [f for f in files if f.rpartition(".")[-1].lower() in cls.IMG_FORMATS]
        if len(images) != len(files):
            other = sorted({f.rpartition(".")[-1].lower() for f in files} - cls.IMG_FORMATS)
            if not images:
                raise NotImplementedError(f"no image files in the source (found suffixes {other}); videos / streams are outside the accelerated path")
            LOGGER.warning(f"WARNING skipping {len(files) - len(images)} non-image file(s) ({other}): videos / streams are outside the accelerated path")
        return images

    @staticmethod
    def decode_image(im):
        """A file path or a PIL image -> contiguous HWC BGR uint8 (loaders.py:488-500: RGB, then channels reversed)."""
        import numpy as np
        from PIL import Image

        if not isinstance(im, Image.Image):
            with Image.open(im) as f:
                im = f.convert("RGB")
        elif im.mode != "RGB":
            im = im.convert("RGB")
        return np.ascontiguousarray(np.asarray(im)[:, :, ::-1])

    def _file_pieces(self, files: List[str], batch: int):
        for lo in range(0, len(files), batch):
            names = files[lo : lo + batch]
            yield lo, [self.decode_image(f) for f in names], names

    # ---- a source larger than one batch (reference predictor.py:221-298, stream_inference: `for self.batch in self.dataset`) -------------------
    def _chunks(self, source, batch: int):
        """``source`` cut into pieces of ``batch`` images: a BCHW float tensor, a uint8 (N, H, W, 3) tensor, or a list of HWC frames."""
        n = len(source)
        for lo in range(0, n, batch):
            yield lo, source[lo : lo + batch], None

    def stream_batches(self, source, batch: int, pieces=None):
        """Generator over the images of ``source``, run ``batch`` at a time, one ``Results`` per image in order.  The device works one batch
        ahead of the host: batch k + 1 is preprocessed and enqueued (its launches, a device copy of batch k's output rows in front of them, an
        asynchronous copy of the kept counts to pinned memory) before batch k's ``Results`` are built, so the host side of postprocess — the
        one synchronisation and a Python object per image — runs under the next batch's kernels.  What the reference's loop does batch by batch
        (predictor.py:246-298), without its per-batch device synchronisations."""
        names = self.model.names
        pending = None

        def finish(item):
            lo, im, rows, counts_host, ev, info, t_pre, t_inf, paths, frames, trows, stash = item
            t0 = time.perf_counter()
            ev.synchronize()
            both = counts_host.tolist()
            counts = both[: rows.shape[0]]
            tracked = (trows, both[rows.shape[0] :]) if trows is not None else None
            out = []
            boxes = self._all_boxes(counts, rows, tracked)
            masks = self._masks_for(stash, counts, rows, im, info)
            for i, k in enumerate(counts):
                one = (info[i] if isinstance(info, list) else info) if info else None
                r = self._result(frames[i] if frames is not None else im[i], paths[i] if paths else f"image{lo + i}.jpg", names, boxes[i],
                                 (one[0], one[1]) if one else im.shape[2:], masks[i])
                out.append(r)
            dt = (time.perf_counter() - t0) * 1e3 / max(len(out), 1)
            for r in out:  # host-side times per image (the device runs ahead: no synchronisation is placed around the stages)
                r.speed = {"preprocess": t_pre, "inference": t_inf, "postprocess": dt}
            return out

        for lo, piece, paths in (pieces if pieces is not None else self._chunks(source, batch)):
            t0 = time.perf_counter()
            im = self.preprocess(piece)
            t1 = time.perf_counter()
            cf = self.forward_device(im)
            rows = cf.nms.out.clone()  # stream-ordered behind this batch's launches, in front of the next batch's (which overwrite the buffer)
            if self.tracker is not None and rows.shape[0] % self.tracker.streams:
                raise ValueError(f"a batch of {rows.shape[0]} images is no multiple of track_streams = {self.tracker.streams}")
            tracked = self._track_launch(cf)
            counts_dev = torch.cat([cf.nms.count, tracked[1]]) if tracked is not None else cf.nms.count  # one copy for both
            counts_host = torch.empty(counts_dev.shape, dtype=counts_dev.dtype, pin_memory=True)
            counts_host.copy_(counts_dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            t2 = time.perf_counter()
            n = max(im.shape[0], 1)
            item = (lo, im, rows, counts_host, ev, getattr(self, "letterbox_info", None), (t1 - t0) * 1e3 / n, (t2 - t1) * 1e3 / n, paths,
                    piece if paths is not None else None, tracked[0] if tracked is not None else None,  # (file sources keep the decoded frame as the result's orig_img)
                    self._mask_stash(cf, streamed=True))
            if pending is not None:
                yield from finish(pending)
            pending = item
        if pending is not None:
            yield from finish(pending)

    # ---- tiled inference (``tile=``): frames larger than the model input, cut into overlapping tiles on the device ----------------
    def _tile_pieces(self, source):
        """``source`` as pieces (lo, frames, paths) of at most ``batch`` frames; frames: HWC uint8 numpy arrays (or rows of a uint8 NHWC tensor)."""
        from pathlib import Path

        batch = self.args.get("batch")
        is_path = lambda v: isinstance(v, (str, Path))  # noqa: E731
        if is_path(source) or (isinstance(source, (list, tuple)) and len(source) > 0 and all(is_path(v) for v in source)):
            return self._file_pieces(self.list_image_files(source), int(batch or 1))
        if type(source).__module__.startswith("PIL.") or (isinstance(source, (list, tuple)) and len(source) > 0 and type(source[0]).__module__.startswith("PIL.")):
            ims = list(source) if isinstance(source, (list, tuple)) else [source]
            frames = [self.decode_image(im) for im in ims]
            paths = [getattr(im, "filename", "") or f"image{i}.jpg" for i, im in enumerate(ims)]
            b = int(batch or len(frames))
            return ((lo, frames[lo : lo + b], paths[lo : lo + b]) for lo in range(0, len(frames), b))
        if isinstance(source, torch.Tensor):
            if source.dtype != torch.uint8 or source.dim() not in (3, 4) or source.shape[-1] != 3:
                raise NotImplementedError("tile with a float BCHW tensor: tiles are cut from pixels (uint8 HWC frames), not from a letterboxed tensor")
            source = source[None] if source.dim() == 3 else source
        elif type(source).__name__ == "ndarray":
            source = [source] if source.ndim == 3 else list(source)
        elif not isinstance(source, (list, tuple)) or len(source) == 0:
            raise NotImplementedError("tile sources: uint8 HWC BGR frames (list of numpy arrays / uint8 NHWC tensor), image files, PIL images")
        return self._chunks(source, int(batch or len(source)))

    # ---- what a task changes in the cross-tile merge: its buffers and its launch (the oriented-box task overrides both) ----
    def _new_merge_bufs(self, frames: int, k: int):
        """The merge buffers of ``frames`` frames of ``k`` tiles each, kept per frame shape in ``_tile_state``."""
        a = self.args
        return H.TileMergeBuffers(frames, k, int(a["max_det"]), int(a["merge_max_det"]), self.device, fuse=str(a["merge_mode"]).lower() != "suppress")

    def _merge_tiles(self, cf: CompiledForward, offs_d: torch.Tensor, k: int, frame_hw, mbufs):
        """The merge launch behind the recorded pass over the tiles: ``cf.nms`` holds the per-tile rows; returns ``mbufs``, filled."""
        a = self.args
        return H.tile_merge(cf.nms, offs_d, k, frame_hw, self.model.yaml["nc"], float(a["merge_iou"]), str(a["merge_metric"]),
                            bool(a["agnostic_nms"]), int(a["merge_max_det"]), bufs=mbufs, mode=str(a["merge_mode"]))

    def _tile_mask_stash(self, cf: CompiledForward, offs_d: torch.Tensor, k: int, merged):
        """Hook behind the cross-tile merge: what the frame masks of this group are assembled from (None: a detection model)."""
        return None

    def _tile_masks_for(self, stash, counts, frame_hw) -> list:
        """Per frame of a group the (k, oh, ow) masks of the rows of its result, or None."""
        return [None] * len(counts)

    def _tiled_enqueue(self, lo: int, frames, paths):
        """Everything one batch of frames launches — per group of frames of one shape: the slicer, the recorded pass over the (F * K)-tile batch,
        the cross-tile merge and, in track mode, the track step — then ONE asynchronous copy of the merged (and the tracker's) counts."""
        import numpy as np

        from .tiling import tile_offsets

        a = self.args
        tile, t0 = int(a["tile"]), time.perf_counter()
        n = len(frames)
        groups: Dict[Tuple[int, int], List[int]] = {}
        for i in range(n):
            f = frames[i]
            if f.ndim != 3 or f.shape[2] != 3 or f.dtype != (torch.uint8 if isinstance(f, torch.Tensor) else np.uint8):
                raise ValueError("tile sources must be uint8 HWC BGR frames")
            groups.setdefault((int(f.shape[0]), int(f.shape[1])), []).append(i)
        if self.tracker is not None:
            if len(groups) > 1:
                raise NotImplementedError("mode='track' with tile: the frames of a batch must have one shape (they are consecutive time steps)")
            if n % self.tracker.streams:
                raise ValueError(f"a batch of {n} images is no multiple of track_streams = {self.tracker.streams}")
        parts, mcounts, tcounts = [], [], []
        for (hf, wf), idxs in groups.items():
            if isinstance(frames, torch.Tensor):
                stacked = frames[idxs[0] : idxs[-1] + 1].to(self.device, non_blocking=True).contiguous()
            else:
                stacked = torch.from_numpy(np.ascontiguousarray(np.stack([frames[i] for i in idxs]))).to(self.device, non_blocking=True)
            key = (len(idxs), hf, wf)
            st = self._tile_state.get(key)
            if st is None:
                while len(self._tile_state) >= self.max_compiled:
                    self._tile_state.pop(next(iter(self._tile_state)))
                offs = tile_offsets(hf, wf, tile, float(a["tile_overlap"]))
                offs_d = torch.tensor(offs, dtype=torch.int32, device=self.device)
                k = len(offs)
                st = self._tile_state[key] = (offs_d, k, torch.empty((len(idxs) * k, 3, tile, tile), dtype=torch.float32, device=self.device),
                                              self._new_merge_bufs(len(idxs), k))
            offs_d, k, tiles, mbufs = st
            H.tiles_batch(stacked, offs_d, tile, out=tiles)  # a frame no larger than the tile is one tile padded with 114
            self.letterbox_info = None  # every tile is an image of its own to the pass: boxes clipped to the tile
            cf = self.forward_device(tiles)
            merged = self._merge_tiles(cf, offs_d, k, (hf, wf), mbufs)
            tracked = None
            if self.tracker is not None and hasattr(self.tracker, "bufs"):
                tout, tcnt = self.tracker.update_batch(merged.out, merged.count)
                tracked = tout.clone()
                tcounts.append(tcnt)
            # copies that outlive the next batch (and the next group: groups of one size share the buffers)
            parts.append((idxs, (hf, wf), merged.out.clone(), tracked, self._tile_mask_stash(cf, offs_d, k, merged)))
            mcounts.append(merged.count.clone() if len(groups) > 1 else merged.count)
        counts_dev = mcounts + tcounts  # (track mode has one group: the tracker's counts follow the merged counts)
        counts_dev = torch.cat(counts_dev) if len(counts_dev) > 1 else counts_dev[0]
        counts_host = torch.empty(counts_dev.shape, dtype=counts_dev.dtype, pin_memory=True)
        counts_host.copy_(counts_dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return lo, frames, paths, parts, counts_host, ev, (time.perf_counter() - t0) * 1e3 / max(n, 1)

    def _tiled_finish(self, item) -> List[Results]:
        lo, frames, paths, parts, counts_host, ev, t_inf = item
        t0 = time.perf_counter()
        ev.synchronize()  # the batch's only device->host synchronisation
        both = counts_host.tolist()
        names, out, o = self.model.names, [None] * len(frames), 0
        index = [None] * len(frames)
        for idxs, hw, rows, trows, stash in parts:
            counts = both[o : o + len(idxs)]
            o += len(idxs)
            tracked = (trows, both[o : o + len(idxs)]) if trows is not None else None
            boxes = self._all_boxes(counts, rows, tracked)
            masks = self._tile_masks_for(stash, counts, hw)
            for j, i in enumerate(idxs):
                img = frames[i]
                if isinstance(img, torch.Tensor):
                    img = img.cpu().numpy()
                out[i] = self._result(img, paths[i] if paths else f"image{lo + i}.jpg", names, boxes[j], hw, masks[j])
                if self.keeps_track_index:
                    index[i] = self.last_track_index[j]
        if self.keeps_track_index:
            self.last_track_index = index
        dt = (time.perf_counter() - t0) * 1e3 / max(len(out), 1)
        for r in out:
            r.speed = {"preprocess": 0.0, "inference": t_inf, "postprocess": dt}
        return out

    def stream_tiled(self, pieces):
        """Generator over the frames of ``pieces`` in order; as ``stream_batches``, the device works one batch ahead of the host."""
        pending = None
        for lo, frames, paths in pieces:
            item = self._tiled_enqueue(lo, frames, paths)
            if pending is not None:
                yield from self._tiled_finish(pending)
            pending = item
        if pending is not None:
            yield from self._tiled_finish(pending)

    def __call__(self, source, stream: bool = False):
        from pathlib import Path

        if self.args.get("tile") is not None:
            gen = self.stream_tiled(self._tile_pieces(source))
            return gen if stream else list(gen)
        is_path = lambda v: isinstance(v, (str, Path))  # noqa: E731
        if is_path(source) or (isinstance(source, (list, tuple)) and len(source) > 0 and all(is_path(v) for v in source)):
            # image files: the reference's loader hands over `batch` files at a time (default 1: every image letterboxed to ITS minimum rectangle)
            files = self.list_image_files(source)
            gen = self.stream_batches(None, 0, pieces=self._file_pieces(files, int(self.args.get("batch") or 1)))
            return gen if stream else list(gen)
        if type(source).__module__.startswith("PIL.") or (isinstance(source, (list, tuple)) and len(source) > 0 and type(source[0]).__module__.startswith("PIL.")):
            ims = list(source) if isinstance(source, (list, tuple)) else [source]  # LoadPilAndNumpy: ONE batch of all of them
            paths = [getattr(im, "filename", "") or f"image{i}.jpg" for i, im in enumerate(ims)]
            gen = self.stream_batches(None, 0, pieces=iter([(0, [self.decode_image(im) for im in ims], paths)]))
            return gen if stream else list(gen)
        batch = self.args.get("batch")
        many = (isinstance(source, (list, tuple)) and len(source) > 0 and getattr(source[0], "ndim", 0) == 3) or (isinstance(source, torch.Tensor) and source.dim() == 4)
        if batch and many and len(source) > int(batch):  # more images than one batch: the reference's dataset loop
            gen = self.stream_batches(source, int(batch))
            return gen if stream else list(gen)
        prof = [ops.Profile(device=self.device) for _ in range(3)]
        with prof[0]:
            im = self.preprocess(source)
        with prof[1]:
            cf = self.forward_device(im)
        with prof[2]:
            results = self.postprocess(cf, im)
        n = max(len(results), 1)
        for r in results:
            r.speed = {"preprocess": prof[0].dt * 1e3 / n, "inference": prof[1].dt * 1e3 / n,
                       "postprocess": prof[2].dt * 1e3 / n}
        if self.args["verbose"]:
            LOGGER.info(f"{len(results)} images: " + ", ".join(f"{len(r)} boxes" for r in results))
        return iter(results) if stream else results


class SegmentationPredictor(DetectionPredictor):
    """Predictor of the segmentation models — reference models/yolo/segment/predict.py:8-74 (``retina_masks`` as there, default False).

    The recorded pass is the detection pass plus Proto, the per-level coefficient branches and — between the NMS and the box rescale, as
    ops.process_mask crops with the boxes in input-image pixels — ``dy_mask_gather``.  The masks need the kept counts on the host (the
    output holds sum(counts) masks), so ``dy_process_mask`` is launched where the counts are read back anyway: one launch per batch, still
    one synchronisation.  The prototypes and the side buffer live in the recorded plan and are overwritten by its next replay; a streamed
    run, whose device works a batch ahead, therefore takes stream-ordered copies of both (and of the counts the kernel bounds its reads by)
    behind the batch's launches, where the detection rows are copied too; a single call assembles from the plan's own buffers.

    ``tile=`` and ``mode="track"`` run on pixel sources.  Tiled: the owner map behind the merge, copies of the tiles' prototypes,
    side rows and counts per batch in flight, one ``dy_tile_process_mask`` launch per frame-shape group in ``_tiled_finish``; masks at
    1 / ``tile_mask_stride`` of the frame.  Tracked: ``last_track_index`` holds per image of the last batch the detection every result row came
    from; the side rows are gathered by it (``dest`` scattered from it with ``tile=``), so a track carries the mask of its detection."""

    def __init__(self, model, overrides: Optional[dict] = None):
        a = overrides or {}
        self.refuse_args(a, model)  # before anything touches the device
        super().__init__(model, overrides)
        self.args["task"] = "segment"
        self.last_track_index: list = []

    keeps_track_index = True

    @staticmethod
    def refuse_args(a: dict, model=None) -> None:
        """What a segmentation predictor does not take, by argument (YOLO.predict asks before it builds one)."""
        if a.get("augment") not in (None, False):
            raise NotImplementedError("augment: not built for segmentation models")
        if a.get("tile") is not None:
            if a.get("retina_masks"):
                raise NotImplementedError("retina_masks with tile: frame masks at full resolution are tile_mask_stride=1")
            strides = getattr(model, "stride", None)
            if strides is not None and float(min(strides)) != 8.0:  # Proto runs at half the finest level: stride 8 -> a quarter of the tile
                raise NotImplementedError(f"tile with a segmentation model whose finest level has stride {float(min(strides)):g} (the P2 -seg models): its "
                                          "prototypes are not a quarter of the tile, which is what the frame masks are built for")
            if a.get("tile_mask_stride", 4) not in H.TILE_MASK_STRIDES or isinstance(a.get("tile_mask_stride", 4), bool):
                raise ValueError(f"tile_mask_stride = {a.get('tile_mask_stride')}, expected one of {H.TILE_MASK_STRIDES}")

    def preprocess(self, im) -> torch.Tensor:
        out = super().preprocess(im)
        if self.args["retina_masks"] and isinstance(self.letterbox_info, list):
            raise NotImplementedError("retina_masks with sources of different shapes in one batch: the masks of a batch share one size")
        return out

    def _tile_mask_stash(self, cf: CompiledForward, offs_d: torch.Tensor, k: int, merged):
        # the owner map behind the merge, and stream-ordered copies of what the next batch's pass overwrites: F * K * mh * mw * 128 bytes of
        # prototypes (13 MB per 1280-pixel tile) per batch in flight, the side rows and the per-tile counts
        a = self.args
        if tuple(cf.protos.shape[2:]) != (int(a["tile"]) // 4,) * 2:  # (a P2 head's Proto runs at half the input: not built)
            raise NotImplementedError(f"tile with a segmentation model whose prototypes are {tuple(cf.protos.shape[2:])} on a {a['tile']}-pixel tile: "
                                      "frame masks are built for prototypes at a quarter of the tile")
        owner = H.tile_mask_owner(cf.nms, offs_d, k, merged, float(a["merge_iou"]), str(a["merge_metric"]), bool(a["agnostic_nms"]),
                                  stitch=str(a["merge_mode"]).lower() != "suppress")
        return cf.protos.clone(), cf.side.clone(), cf.nms.count.clone(), owner, offs_d

    def _tile_masks_for(self, stash, counts, frame_hw) -> list:
        protos, side, tcount, owner, offs_d = stash
        f, m, tile = len(counts), int(self.args["merge_max_det"]), int(self.args["tile"])
        # dest: the output mask of every kept row -- the rows of the frame's result in their order (the tracker's idx where it returned rows)
        dest = torch.full((f, m), -1, dtype=torch.int32, device=self.device)
        total, spans = 0, []
        for j in range(f):
            idx = self.last_track_index[j]
            n = int(idx.numel())
            if n:
                dest[j, idx.to(self.device)] = torch.arange(total, total + n, dtype=torch.int32, device=self.device)
            spans.append((total, n))
            total += n
        if total == 0:
            return [None] * f
        allm = H.tile_process_mask(protos, side, tcount, offs_d, owner, dest, total, (tile, tile), frame_hw, int(self.args["tile_mask_stride"]))
        return [allm[o : o + n] if n else None for o, n in spans]

    def _record_masks(self, cf: CompiledForward, aux) -> None:
        if not (isinstance(aux, tuple) and len(aux) == 3):
            raise RuntimeError("SegmentationPredictor needs a model whose head is Segment")
        _, levels, protos = aux
        cf.protos = protos
        cf.side = H.mask_gather(cf.nms, levels=levels)

    def _mask_stash(self, cf: CompiledForward, streamed: bool):
        if streamed:
            return cf.protos.clone(), cf.side.clone(), cf.nms.count.clone()
        return cf.protos, cf.side, cf.nms.count

    def _masks_for(self, stash, counts, rows, im, info) -> list:
        protos, side, count = stash
        n, _, mh, mw = protos.shape
        if self.tracker is not None:
            # a track carries the mask of the detection it matched (trackers/track.py: results[i][idx]): the side rows (and the retina form's
            # crop rows) are gathered by the tracker's idx in front of the assembly -- 36 floats a row, not a mask copy
            # (one padded index per batch, one gather per buffer)
            counts = [int(idx.numel()) for idx in self.last_track_index]
            pad = torch.nn.utils.rnn.pad_sequence(list(self.last_track_index) + [torch.zeros(side.shape[1], dtype=torch.long, device=side.device)], batch_first=True)[:n]
            side = torch.gather(side, 1, pad[:, :, None].expand(-1, -1, side.shape[2]))
            rows = torch.gather(rows, 1, pad[:, :, None].expand(-1, -1, rows.shape[2]))
            count = torch.tensor(counts, dtype=torch.int32, pin_memory=True).to(self.device, non_blocking=True)
        ih, iw = int(im.shape[2]), int(im.shape[3])
        if self.args["retina_masks"]:
            h0, w0 = (info[0], info[1]) if info else (ih, iw)
            # scale_masks (utils/ops.py:732-753): the letterbox-free window of the proto grid, resized to the original image
            gain = min(mh / h0, mw / w0)
            pad_w, pad_h = (mw - w0 * gain) / 2, (mh - h0 * gain) / 2
            top, left = int(pad_h), int(pad_w)
            win = (top, left, int(mh - pad_h) - top, int(mw - pad_w) - left)
            allm = H.process_mask(protos, side, count, counts, (h0, w0), windows=[win] * n, crop_rows=rows)
        else:
            allm = H.process_mask(protos, side, count, counts, (ih, iw), ratio=(mw / iw, mh / ih))
        out, o = [], 0
        for k in counts:
            out.append(allm[o : o + k] if k else None)
            o += k
        return out


class OBBPredictor(DetectionPredictor):
    """Predictor of the oriented-box models -- reference models/yolo/obb/predict.py:8-46.

    The recorded pass is the detection pass (every Detect fusion and the fused candidate filter unchanged: the filter does not look at boxes)
    plus the per-level angle branches and ``dy_obb_decode`` inside the head, then ``dy_nms_rotated`` in place of ``dy_nms`` and
    ``dy_scale_rboxes`` in place of ``dy_scale_boxes``; one synchronisation per batch, and a streamed run copies the (N, max_det, 7) rows
    behind the batch's launches as it copies detection rows.  ``Results.obb`` carries the rows; ``Results.boxes`` is None.
    ``mode="track"``: the rotated track step reads the same rows; a tracked image's ``Results.obb`` has 8 columns.

    ``tile=``: the tiled loop is the detection task's; the cross-tile merge is ``dy_tile_merge_rotated`` -- greedy suppression
    at ``merge_iou`` as a ProbIoU threshold.  An IoS-like measure and fusing merges are not built for rotated boxes."""

    @staticmethod
    def refuse_tile_args(a: dict) -> None:
        """What ``tile=`` does not do for oriented boxes, refused by argument name (also by ``YOLO.predict``, before a predictor is built)."""
        if a.get("tile") is None:
            return
        if str(a.get("merge_metric", "iou")).lower() != "iou":
            raise NotImplementedError(f"merge_metric = '{a['merge_metric']}': the oriented-box tile merge compares with ProbIoU (merge_metric='iou' only)")
        if str(a.get("merge_mode", "suppress")).lower() != "suppress":
            raise NotImplementedError(f"merge_mode = '{a['merge_mode']}': fusing merges are not built for oriented boxes (merge_mode='suppress' only)")

    def __init__(self, model, overrides: Optional[dict] = None):
        a = overrides or {}
        if a.get("augment") not in (None, False):  # before anything touches the device
            raise NotImplementedError("augment: not built for oriented-box models")
        self.refuse_tile_args(a)
        super().__init__(model, overrides)
        self.args["task"] = "obb"

    rotated_rows = True

    def make_tracker(self):
        """The rotated tracker (``dy_track_step_rotated`` or the host class with ``rotated=True``) behind ``dy_nms_rotated`` + ``dy_scale_rboxes``."""
        if self.args["tile"] is not None:
            raise NotImplementedError("track with tile: not built for oriented-box models")
        return super().make_tracker()

    def _new_nms_bufs(self, nb: int, anchors: int):
        return H.RNmsBuffers(nb, anchors, int(self.args["max_det"]), self.device)

    def _record_nms(self, y, aux, bufs):
        if not (isinstance(aux, tuple) and len(aux) == 3 and isinstance(aux[1], torch.Tensor)):
            raise RuntimeError("OBBPredictor needs a model whose head is OBB")
        a = self.args
        return H.nms_rotated(y, aux[1], float(a["conf"]), float(a["iou"]), max_det=int(a["max_det"]), max_nms=int(a["max_nms"]),
                             max_wh=float(a["max_wh"]), agnostic=bool(a["agnostic_nms"]), nc=self.model.yaml["nc"],
                             classes_mask=self._classes_mask, bufs=bufs, prefiltered=bufs is not None)

    def _record_scale(self, cf: CompiledForward, params: torch.Tensor) -> None:
        H.scale_rboxes_(cf.nms, params)

    def _result(self, img, path, names, rows, orig_shape, masks) -> Results:
        return Results(img, path, names, obb=rows, orig_shape=orig_shape)

    def _new_merge_bufs(self, frames: int, k: int):
        return H.RTileMergeBuffers(frames, k, int(self.args["max_det"]), int(self.args["merge_max_det"]), self.device)

    def _merge_tiles(self, cf: CompiledForward, offs_d: torch.Tensor, k: int, frame_hw, mbufs):
        a = self.args
        return H.tile_merge_rotated(cf.nms, offs_d, k, frame_hw, self.model.yaml["nc"], float(a["merge_iou"]), bool(a["agnostic_nms"]),
                                    int(a["merge_max_det"]), bufs=mbufs)


class PosePredictor(DetectionPredictor):
    """Predictor of the pose models -- reference models/yolo/pose/predict.py:8-53.

    The recorded pass is the detection pass (every Detect fusion and the fused candidate filter unchanged) plus the per-level keypoint
    branches, then ``dy_nms``, ``dy_kpt_decode`` in its gather form (the keypoints of the kept anchors only), ``dy_scale_boxes`` and
    ``dy_scale_coords``; one synchronisation per batch, and a streamed run copies the (N, max_det, nk) keypoint rows behind the batch's
    launches where it copies the detection rows.  ``Results.boxes`` as for detection, ``Results.keypoints.data`` (n, *kpt_shape) fp32 on the
    device.  ``track``, ``tile=`` and ``augment=True`` are refused.

    ``predict_crops`` (``YOLO.predict(frames, crops=boxes)``): every box of every frame becomes an expanded integer window of
    its frame, letterboxed to ``imgsz x imgsz`` by ONE ``dy_crops_letterbox_u8_to_nchw_f32`` launch per batch of crops and run through the
    recorded pass; boxes and keypoints are clamped to the crop and moved to frame pixels by ``dy_scale_coords``' offset."""

    def __init__(self, model, overrides: Optional[dict] = None):
        a = overrides or {}
        self.refuse_args(a)  # before anything touches the device
        super().__init__(model, overrides)
        self.args["task"] = "pose"
        head = self.model.model[-1]
        if not hasattr(head, "kpt_shape"):
            raise RuntimeError("PosePredictor needs a model whose head is Pose")
        self.kpt_shape = (int(head.kpt_shape[0]), int(head.kpt_shape[1]))
        self._crop_off = None  # predict_crops: per image of the batch the (x0, y0) of its window
        self._crop_bufs: Dict[int, torch.Tensor] = {}

    @staticmethod
    def refuse_args(a: dict) -> None:
        """What a pose predictor does not take, by argument (YOLO.predict asks before it builds one)."""
        if a.get("augment") not in (None, False):
            raise NotImplementedError("augment: not built for pose models")
        if a.get("tile") is not None:
            raise NotImplementedError("tile: not built for pose models")

    @staticmethod
    def check_crops(source, boxes, expand: float):
        """The host checks of ``crops=``: (frames, rects) or ``ValueError`` -- nothing here touches a device."""
        from .crops import as_frames, crop_rects

        frames = as_frames(source)
        return frames, crop_rects(frames, boxes, expand)

    def make_tracker(self):
        raise NotImplementedError("track: not built for pose models")

    def preprocess(self, im) -> torch.Tensor:
        self._crop_off = None
        return super().preprocess(im)

    def _kpt_params(self, h: int, w: int, n: int):
        """Per image (gain, pad_x, pad_y, clip_w, clip_h, off_x, off_y) of ops.scale_coords (utils/ops.py:756-788; the pads unrounded, in
        Python floats) for the current source: n rows."""
        info = getattr(self, "letterbox_info", None)
        if info is None:
            return [[1.0, 0.0, 0.0, float(w), float(h), 0.0, 0.0]] * n
        off = self._crop_off or [(0, 0)] * n
        rows = []
        for (h0, w0, hn, wn), (ox, oy) in zip((info if isinstance(info, list) else [info] * n), off):
            gain = min(hn / h0, wn / w0)
            rows.append([gain, (wn - w0 * gain) / 2, (hn - h0 * gain) / 2, float(w0), float(h0), float(ox), float(oy)])
        return rows

    def _record_masks(self, cf: CompiledForward, aux) -> None:
        if not (isinstance(aux, tuple) and len(aux) == 2 and isinstance(aux[1], (list, tuple))):
            raise RuntimeError("PosePredictor needs a model whose head is Pose")
        head = self.model.model[-1]
        cf.kpts = H.kpt_gather(cf.nms, aux[1], [float(s) for s in head.stride], self.kpt_shape)

    def _record_scale(self, cf: CompiledForward, params: torch.Tensor) -> None:
        H.scale_boxes_(cf.nms, params)
        n = cf.nms.batch
        cf.kpt_key = self._kpt_params(self._recording_hw[0], self._recording_hw[1], n)
        cf.kpt_params = torch.tensor(cf.kpt_key, dtype=torch.float32, device=self.device)
        H.scale_coords_(cf.kpts, cf.nms.count, cf.kpt_params, self.kpt_shape, boxes=cf.nms.out)

    def _record(self, im: torch.Tensor) -> CompiledForward:
        self._recording_hw = (int(im.shape[2]), int(im.shape[3]))
        return super()._record(im)

    def forward_device(self, im: torch.Tensor) -> CompiledForward:
        cf = self._compiled.get((tuple(im.shape), self.dtype))
        if cf is not None and hasattr(cf, "kpt_params"):  # the recorded dy_scale_coords launch reads this device tensor: refresh it when the source geometry changed
            kp = self._kpt_params(im.shape[2], im.shape[3], im.shape[0])
            if kp != cf.kpt_key:
                cf.kpt_params.copy_(torch.tensor(kp, dtype=torch.float32))
                cf.kpt_key = kp
        return super().forward_device(im)

    def _mask_stash(self, cf: CompiledForward, streamed: bool):
        return cf.kpts.clone()  # (the next pass overwrites the plan's buffer: the Results keep views of this copy, as of the rows')

    def _masks_for(self, stash, counts, rows, im, info) -> list:
        return [stash[i, :k].view(k, *self.kpt_shape) for i, k in enumerate(counts)]

    def _result(self, img, path, names, rows, orig_shape, masks) -> Results:
        from .results import Keypoints

        shape = tuple(orig_shape)
        return Results(img, path, names, boxes=rows, orig_shape=shape, keypoints=Keypoints(masks, shape, masked=True))

    # ---- person crops of frames ----
    def predict_crops(self, source, boxes):
        """Generator: one ``Results`` per crop, frame by frame in box order; ``Results.crop = (frame, x0, y0, x1e, y1e)``, boxes and keypoints
        in frame pixels, ``orig_shape`` the frame's.  All crops of the call run ``batch`` at a time: one slicer launch, one recorded pass and
        one synchronisation per batch, the device one batch ahead of the host."""
        import numpy as np

        from .crops import crop_table

        frames, rects = self.check_crops(source, boxes, float(self.args.get("crop_expand", 0.2)))  # (ValueError before any device use)
        size = int(self.args.get("imgsz", 640))
        table = torch.from_numpy(crop_table(rects, size, int(self.model.stride.max())))
        stacked = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(self.device, non_blocking=True)
        hw = tuple(frames[0].shape[:2])
        b = int(self.args.get("batch") or len(rects))
        names = self.model.names

        def finish(item):
            lo, rows, kpts, counts_host, ev = item
            ev.synchronize()  # the batch's only device->host synchronisation
            out = []
            for i, k in enumerate(counts_host.tolist()):
                rect = rects[lo + i]
                r = self._result(frames[rect[0]], f"image{rect[0]}.jpg", names, rows[i, :k], hw, kpts[i, :k].view(k, *self.kpt_shape))
                r.crop = rect
                out.append(r)
            return out

        pending = None
        for lo in range(0, len(rects), b):
            t = table[lo : lo + b].contiguous()
            n = int(t.shape[0])
            buf = self._crop_bufs.get(n)
            if buf is None or tuple(buf.shape[2:]) != (size, size):
                buf = self._crop_bufs[n] = torch.empty((n, 3, size, size), dtype=torch.float32, device=self.device)
            self.letterbox_info = [(int(r[4]), int(r[3]), size, size) for r in t.tolist()]
            self._crop_off = [(int(r[1]), int(r[2])) for r in t.tolist()]
            H.crops_letterbox(stacked, t, size, size, out=buf)
            cf = self.forward_device(buf)
            rows, kpts = cf.nms.out.clone(), cf.kpts.clone()  # stream-ordered behind this batch's launches, in front of the next batch's
            counts_host = torch.empty(cf.nms.count.shape, dtype=cf.nms.count.dtype, pin_memory=True)
            counts_host.copy_(cf.nms.count, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            if pending is not None:
                yield from finish(pending)
            pending = (lo, rows, kpts, counts_host, ev)
        if pending is not None:
            yield from finish(pending)
