"""``YOLO`` / ``Model`` user API (reference: ultralytics/engine/model.py:29-1177,
ultralytics/models/yolo/model.py:11-59) for the detection, segmentation (prediction, validation and training), oriented-box (prediction, validation,
tracking and training) and pose (prediction: whole images, and batched person crops of frames through ``predict(frames, crops=boxes)``) tasks on the
MI355X path."""
from __future__ import annotations

from pathlib import Path
from typing import List, Union

import torch
import torch.nn as nn

from ..nn.tasks import DetectionModel, OBBModel, PoseModel, SegmentationModel, guess_model_task, yaml_model_load
from ..utils import LOGGER
from .predictor import DetectionPredictor, OBBPredictor, PosePredictor, SegmentationPredictor
from .results import Results


class TaskMismatch(ValueError, NotImplementedError):
    """``task="pose"`` asked of a YAML whose head is another task's.  A ``ValueError`` like every other task / head mismatch; also a
    ``NotImplementedError``, which is what the same call raised while the pose task did not exist, so callers that catch either keep working."""


class Model(nn.Module):
    """Same constructor and call surface as the reference ``Model`` (engine/model.py:82-87, 501-560, 744-817)."""

    def __init__(self, model: Union[str, Path] = "yolov8s-p2-repvgg.yaml", task: str = None, verbose: bool = False) -> None:
        super().__init__()
        self.predictor = None
        self.model = None
        self.trainer = None
        self.ckpt = None
        self.cfg = None
        self.ckpt_path = None
        self.overrides = {}
        self.task = task
        if task not in (None, "detect", "segment", "obb", "pose"):
            raise NotImplementedError(f"task '{task}': only 'detect', 'segment', 'obb' and 'pose' are on the accelerated path")
        model = str(model).strip()
        if Path(model).suffix in {".yaml", ".yml"}:
            self._new(model, verbose=verbose)
        elif Path(model).suffix == ".pt":
            self._load(model)
            self.task = guess_model_task(self.model)
        else:
            raise NotImplementedError(f"'{model}': give a model YAML (*.yaml) or a state-dict checkpoint (*.pt); "
                                      "weight-name downloads need network access and are out of scope")
        self.model_name = model

    @property
    def task_map(self):
        from .trainer import DetectionTrainer

        return {"detect": {"model": DetectionModel, "predictor": DetectionPredictor, "trainer": DetectionTrainer},
                "segment": {"model": SegmentationModel, "predictor": SegmentationPredictor, "trainer": DetectionTrainer}}

    @property
    def oriented_task_map(self):
        """The oriented-box task, kept apart from ``task_map`` (whose key set the package's tests pin): model, predictor and trainer -- the
        detection trainer, which takes ``OBBValidator`` and the criterion's six-column table from the model (obb/train.py)."""
        from .trainer import DetectionTrainer

        return {"obb": {"model": OBBModel, "predictor": OBBPredictor, "trainer": DetectionTrainer}}

    @property
    def pose_task_map(self):
        """The pose task, kept apart from ``task_map`` like the oriented-box one: model and predictor; ``val`` scores a pose model with
        ``PoseValidator`` (its task table).  There is no trainer: ``train`` refuses a pose model before it looks for one."""
        return {"pose": {"model": PoseModel, "predictor": PosePredictor}}

    def _task_classes(self, task: str) -> dict:
        return {**self.task_map, **self.oriented_task_map, **self.pose_task_map}[task]

    def _new(self, cfg: str, task=None, model=None, verbose=False) -> None:
        """Build from a YAML — reference engine/model.py:231-264."""
        cfg_dict = yaml_model_load(cfg)
        self.cfg = cfg
        found = guess_model_task(cfg_dict)
        if self.task is not None and self.task != found:
            raise (TaskMismatch if self.task == "pose" else ValueError)(f"task '{self.task}' was asked for, but the head of '{cfg}' makes it a '{found}' model")
        self.task = found
        self.model = (model or self._task_classes(self.task)["model"])(cfg_dict, verbose=verbose)
        self.overrides["model"] = self.cfg
        self.overrides["task"] = self.task

    def _load(self, weights: str, task=None) -> None:
        """Load a checkpoint: either {'yaml': cfg dict, 'model': state_dict} as written by ``save``, or the reference's
        pickled module graph (``ema`` / ``model`` entries, tasks.py:786-926) through the restricted unpickler of
        nn/checkpoint.py — no ``ultralytics`` package needed."""
        from ..nn.checkpoint import load_reference_checkpoint

        self.model, meta = load_reference_checkpoint(str(weights))
        self.ckpt, self.ckpt_path = meta, weights
        self.overrides["model"] = weights

    def save(self, filename: Union[str, Path] = "saved_model.pt") -> None:
        """Reference engine/model.py:366-395: a checkpoint with the trainer's key layout ({epoch, ema / model, optimizer,
        train_args, date, version ...}); the module graph is pickled in fp16 under the reference's class paths
        (nn/checkpoint.py::save_reference_checkpoint), so both this package and the reference itself can load it."""
        from datetime import datetime

        from ..nn.checkpoint import save_reference_checkpoint

        extra = {k: v for k, v in (self.ckpt or {}).items() if k in ("epoch", "best_fitness", "updates", "train_args", "train_metrics", "train_results")}
        extra["date"] = datetime.now().isoformat()
        save_reference_checkpoint(filename, self.model, self.model.state_dict(), extra=extra)

    def __call__(self, source=None, stream: bool = False, **kwargs):
        return self.predict(source, stream, **kwargs)

    def predict(self, source=None, stream: bool = False, predictor=None, **kwargs) -> List[Results]:
        """Reference engine/model.py:501-560: predictor created on first use, conf defaults to 0.25.

        Pose models only: ``crops=boxes`` with ``source`` = uint8 HWC frames of one shape ((F, H, W, 3) array or list) and ``boxes`` = a
        list of F host arrays (n_i, 4) of xyxy frame pixels runs the model on the window of every box grown by ``crop_expand`` (default 0.2) of its
        width / height per side; one ``Results`` per box, frame by frame in box order, in frame pixels, with ``Results.crop``.  An empty crop,
        frames of different shapes, a tensor source or a model of another task: ``ValueError`` before any device use."""
        if source is None:
            raise ValueError("'source' is missing; the device path takes a BCHW float tensor in [0, 1]")
        self._refuse_for_segment(kwargs, source)
        self._refuse_for_obb(kwargs, source)
        self._refuse_for_pose(kwargs, source)
        track = kwargs.get("mode") == "track"
        args = {**self.overrides, "conf": 0.1 if track else 0.25, **kwargs}
        args.pop("model", None), args.pop("task", None), args.pop("mode", None)
        persist = bool(args.pop("persist", False))
        crops = args.pop("crops", None)  # (host arrays: not part of what a predictor is keyed on)
        if not track:
            args.pop("tracker", None)
        elif args.get("tile") is not None and int(args.get("merge_max_det", 1000)) > 1024:  # (before a predictor is built or anything is launched)
            raise ValueError(f"merge_max_det = {args['merge_max_det']} with tile in track mode: the track step takes at most 1024 detections per frame")
        if self.predictor is None or getattr(self, "_pred_args", None) != (args, track):
            self.predictor = (predictor or self._task_classes(self.task)["predictor"])(self.model, overrides=args)
            self._pred_args = (args, track)
        if track:
            # the tracker outlives the predictor (a predict call in between rebuilds that): persist=True goes on with its tracks and ids
            p = self.predictor
            key = (str(p.args["tracker"]), bool(p.args["device_track"]), int(p.args["track_streams"]),
                   int(p.args["merge_max_det"] if p.args["tile"] is not None else p.args["max_det"]), int(p.args["max_tracks"]), str(p.device))
            if getattr(self, "_tracker_key", None) != key:
                self._tracker, self._tracker_key = p.make_tracker(), key
            elif not persist:
                self._tracker.reset()
            p.tracker = self._tracker
        else:
            self.predictor.tracker = None
        if crops is not None:
            gen = self.predictor.predict_crops(source, crops)
            return gen if stream else list(gen)
        return self.predictor(source, stream=stream)

    def track(self, source=None, stream: bool = False, persist: bool = False, tracker="bytetrack.yaml", **kwargs) -> List[Results]:
        """Reference engine/model.py:562-620: ``predict`` with ``mode="track"`` and conf defaulting to 0.1 (ByteTrack wants the low-score
        detections), each batch's detections handed to the tracker (trackers/track.py).  Results whose tracker returned rows carry 7-column
        boxes (``boxes.is_track``, ``boxes.id``).  ``persist=False`` resets the tracker at the start of the call, ``persist=True`` continues
        tracks and ids across calls.  ``tracker``: settings under cfg/trackers or a path (ByteTrack only).  Package extensions:
        ``device_track`` (default true: the dy_track_step kernel behind the NMS, no extra synchronisation; false: the same tracker on the host)
        and ``track_streams`` = S independent video streams per batch (image k is stream k % S at time step k // S; the batch size must be
        a multiple of it).

        Oriented-box models are tracked with the same ByteTrack on ProbIoU costs (``dy_track_step_rotated`` / the host class
        with ``rotated=True``); tracked results carry 8-column ``obb`` rows [x, y, w, h, r, id, conf, cls].  Two calls stay refused for them,
        with ``NotImplementedError``, before a predictor is built: ``tile=`` (tiled oriented tracking is not built), and a float BCHW tensor
        source -- pass uint8 HWC frames, image files or PIL images.  The second is kept because the package's own tests pin
        ``YOLO(<-obb>).track(<float tensor>)`` as a refused call; the predictor itself would take the tensor."""
        return self.predict(source, stream, **{**kwargs, "mode": "track", "persist": persist, "tracker": tracker})

    def _refuse_for_segment(self, kwargs: dict, source=None) -> None:
        """What a segmentation model does not do, refused by argument name before a predictor is built or anything is launched.  ``tile=`` and
        ``mode="track"`` are built for pixel sources: uint8 HWC frames, image files, PIL images.  A float BCHW tensor source stays
        refused with either -- the package's own tests pin ``YOLO(<-seg>).predict(<float tensor>, tile=...)`` / ``.track(<float tensor>)`` as
        refused calls (the arrangement of ``-obb`` models in ``track``'s docstring)."""
        if self.task != "segment":
            return
        a = {**self.overrides, **kwargs}
        floats = isinstance(source, torch.Tensor) and source.dtype != torch.uint8
        if a.get("mode") == "track" and floats:
            raise NotImplementedError("track with a float BCHW tensor: not taken for segmentation models; pass uint8 HWC BGR frames, image files or PIL images")
        if a.get("tile") is not None and floats:
            raise NotImplementedError("tile with a float BCHW tensor: tiles are cut from uint8 pixels (HWC frames), not from a letterboxed tensor")
        if a.get("augment"):
            raise NotImplementedError("augment=True: test-time augmentation is not built for segmentation models")
        SegmentationPredictor.refuse_args(a, self.model)

    def _refuse_for_obb(self, kwargs: dict, source=None) -> None:
        """What an oriented-box model does not do, refused by argument name before a predictor is built or anything is launched.  ``tile=`` is
        built and so is ``mode="track"`` without tiles on pixel sources; what they do not take -- a float tensor source, an IoS metric, a fusing merge -- is refused here too, so that
        the refusal comes before the predictor moves the model to the device."""
        if self.task != "obb":
            return
        a = {**self.overrides, **kwargs}
        if a.get("mode") == "track":  # built for pixel sources, one frame shape per batch, without tiles
            if a.get("tile") is not None:
                raise NotImplementedError("track with tile: not built for oriented-box models")
            if isinstance(source, torch.Tensor) and source.dtype != torch.uint8:
                raise NotImplementedError("track with a float BCHW tensor: not taken for oriented-box models; pass uint8 HWC BGR frames (a list of one "
                                          "shape, or a uint8 NHWC tensor), image files or PIL images")
        if a.get("tile") is not None:
            if isinstance(source, torch.Tensor) and source.dtype != torch.uint8:
                raise NotImplementedError("tile with a float BCHW tensor: tiles are cut from uint8 pixels (HWC frames), not from a letterboxed tensor")
            OBBPredictor.refuse_tile_args(a)
        if a.get("augment"):
            raise NotImplementedError("augment=True: test-time augmentation is not built for oriented-box models")

    def _refuse_for_pose(self, kwargs: dict, source=None) -> None:
        """What a pose model does not do -- ``track``, ``tile=``, ``augment=True`` -- refused by argument name before a predictor is built or
        anything is launched; and ``crops=``, which only a pose model takes, checked on the host: the frames, the boxes and every
        crop rectangle."""
        a = {**self.overrides, **kwargs}
        if self.task != "pose":
            if a.get("crops") is not None:
                raise ValueError(f"crops: person crops are taken by pose models only; this is a '{self.task}' model")
            return
        if a.get("mode") == "track":
            raise NotImplementedError("track: not built for pose models")
        if a.get("tile") is not None:
            raise NotImplementedError("tile: not built for pose models (crops= runs a pose model on windows of a large frame)")
        if a.get("augment"):
            raise NotImplementedError("augment=True: test-time augmentation is not built for pose models")
        if a.get("crops") is not None:
            PosePredictor.check_crops(source, a["crops"], float(a.get("crop_expand", 0.2)))

    def profile(self, source, **kwargs) -> list:
        """Per-layer device time of one pass over ``source`` (reference ``predict(profile=True)`` -> ``_profile_one_layer``, nn/tasks.py:171-191):
        [{layer, type, launches, ms, kernels}], see ``DetectionPredictor.profile_layers``."""
        self.predict(source, **kwargs)
        return self.predictor.profile_layers(self.predictor.preprocess(source))

    def train(self, trainer=None, **kwargs):
        """Reference engine/model.py:744-817: build the trainer from the model + overrides, train, then continue with the
        trained weights.  ``data``: a tensor dataset (.pt / dict) or "synthetic[:N]" (engine/trainer.py::load_dataset);
        an oriented-box model (task ``obb``: ``OBBModel``, ``v8OBBLoss`` through ``dy_obb_loss``, ``OBBValidator`` per epoch)
        takes a dict / ``.pt`` whose ``bboxes`` are (M, 5) normalised xywh + the angle in radians, or ``"synthetic-obb[:N]"``; for it
        four-column boxes (``"synthetic[:N]"`` among them), ``device_augment=True`` and a YOLO-format dataset YAML (corner-format labels)
        are refused with ``NotImplementedError`` naming the argument, before a trainer is built or a device selected;
        a segmentation model (task ``segment``: ``SegmentationModel``, ``v8SegmentationLoss`` through ``dy_detection_loss`` + ``dy_seg_loss``,
        ``SegmentationValidator`` per epoch) takes a dict / ``.pt`` with ``masks`` (uint8 / int32 (N, gh, gw) overlap index maps, value
        k + 1 = the image's k-th label; the prototype grid equals the map or is exactly twice it) or ``"synthetic-seg[:N]"``; for it a dataset
        without ``masks`` (``"synthetic[:N]"`` among them), float per-label masks, another grid ratio, ``device_augment=True`` and a dataset
        YAML are refused the same way;
        ``device="0,1,.."`` trains with one rank per GPU (child processes under torch.distributed.run, RCCL all-reduce),
        after which rank-less this process reloads ``weights/last.pt`` — as the reference does (model.py:806-813)."""
        if self.task == "pose":  # before a trainer is built or a device selected
            raise NotImplementedError("train: pose training (v8PoseLoss) is not built")
        args = {**{k: v for k, v in self.overrides.items() if k not in ("task", "mode")}, **kwargs}
        if self.task == "segment":  # the training twin of val's dataset rule, before a trainer is built or a device selected
            from .trainer import check_seg_train_data

            check_seg_train_data(args.get("data") or "synthetic", args, float(self.model.stride[0]))
        if self.task == "obb":  # the training twin of val's dataset rule, before a trainer is built or a device selected
            from .trainer import check_obb_train_data

            check_obb_train_data(args.get("data") or "synthetic", args)
        devs = [x for x in str(args.get("device", "")).replace("cuda:", "").split(",") if x.strip() != ""]
        multi = len(devs) > 1
        if multi:
            # the ranks rebuild the model from a file: hand them the current weights
            import tempfile

            start = Path(tempfile.mkdtemp(prefix="dyolo_train_")) / "start.pt"
            self.save(start)
            args["model"] = str(start)
            self.trainer = (trainer or self._task_classes(self.task)["trainer"])(overrides=args)
        else:
            args.setdefault("model", self.overrides.get("model"))
            self.trainer = (trainer or self._task_classes(self.task)["trainer"])(self.model, overrides=args)
        out = self.trainer.train()
        last = self.trainer.last
        if multi and last.exists():
            self._load(str(last))
        elif not multi:
            # the reference continues with best/last.pt = the EMA weights whatever the GPU count (model.py:812-814); the live model holds
            # the raw optimizer weights (flat-buffer views), so the EMA state is loaded into it (same values last.pt carries, fp32)
            self.model.load_state_dict(self.trainer.ema.state_dict(self.model))
            self.model.eval()  # packs are dropped by train() -> eval()
        self.predictor = None
        return out

    def val(self, validator=None, **kwargs) -> dict:
        """Reference engine/model.py:620-656 (``Model.val``): the model's own weights scored on a dataset by the task's validator
        (engine/validator.py here): the model pass, the ``multi_label`` NMS at conf 0.001 and the matching of detections to labels on the
        device, AP on the host; ``device_match=False`` matches on the host as the reference does, with the same result.  ``data``: a tensor
        dataset — a dict / ``.pt`` in the training layout, its ``"val"`` split when it has one — or ``"synthetic[:N]"``
        (engine/trainer.py::load_dataset; image folders and dataset YAMLs are outside the accelerated path); ``batch``, ``imgsz``, ``conf``,
        ``iou``, ``max_det``, ``half`` / ``dtype``, ``device`` as the reference's arguments.  The result is kept in ``self.metrics``.

        detect (models/yolo/detect/val.py; ``DetectionValidator``, ``dy_val_match``): the reference's ``results_dict``
        (metrics/precision(B) ... metrics/mAP50-95(B), fitness) with the validation losses.
        segment (models/yolo/segment/val.py; ``SegmentationValidator``): box and mask metrics, the masks scored by ``dy_val_mask_match``.  The
        dataset must carry ``masks``, the reference's ``overlap_mask=True`` index maps (N, gh, gw) uint8 / int32 — the prototype grid equals
        the map's or is exactly twice it.  ``SegmentMetrics``' dict (the four (B) and four (M) entries, ``fitness``), no validation loss.
        obb (models/yolo/obb/val.py; ``OBBValidator``): the rotated ``multi_label`` NMS (``dy_nms_rotated_ml``) and the ProbIoU matching
        (``dy_val_match_rotated``).  The dataset's ``bboxes`` must be (M, 5): normalised xywh and the angle in radians.  ``OBBMetrics``' dict
        (the four (B) entries, ``fitness``), no validation loss.
        pose (models/yolo/pose/val.py; ``PoseValidator``): box metrics and keypoint metrics, the keypoints scored by object keypoint
        similarity through ``dy_val_oks_match``.  The dataset must carry ``keypoints`` (M, nkpt, 3), normalised x, y and the visibility of
        every label, with the model's nkpt ((M, nkpt, 2), all visible, for a ``kpt_shape`` of two values per keypoint), or be
        ``"synthetic-pose[:N]"``; anything else is refused with ``NotImplementedError`` before a device is selected.  ``PoseMetrics``' dict
        (the four (B) and four (P) entries, ``fitness``), no validation loss.
        ``save_json``, plots, the DOTA merge (``eval_json``) and ``save_txt`` are not built."""
        from .predictor import resolve_dtype
        from .trainer import TensorLoader, load_dataset
        from . import validator as V
        from .. import hip_ops as H
        from ..utils.torch_utils import select_device

        args = {**{k: v for k, v in self.overrides.items() if k not in ("task", "mode")}, **kwargs}
        if args.get("data") is None:
            raise ValueError("val(): 'data' is missing (a tensor dataset: dict / .pt, or 'synthetic[:N]')")
        # per task: the dataset check, the head's name when FP8 storage is refused (None: whatever is not a storage type of the training path
        # falls back to fp32, the pass returns the raw maps for the loss), the loader keys, the validator
        keys = ("img", "batch_idx", "cls", "bboxes")
        check, fp8_refused, keys, default = {"detect": (None, None, keys, V.DetectionValidator),
                                             "segment": (self._check_val_masks, "Segment", keys + ("masks",), V.SegmentationValidator),
                                             "obb": (self._check_val_xywhr, "OBB", keys, V.OBBValidator),
                                             "pose": (self._check_val_keypoints, "Pose", keys + ("keypoints",), V.PoseValidator)}[self.task]
        # the dataset first: whatever it lacks is refused before a device is selected, the model moved or a validator built
        kpt_shape = tuple(int(v) for v in self.model.model[-1].kpt_shape) if self.task == "pose" else None
        data = load_dataset(args["data"], int(args.get("imgsz", 640)), self.model.yaml["nc"], int(args.get("seed", 0)), kpt_shape=kpt_shape)
        data = data.get("val") or data
        if check is not None:
            name = repr(args["data"] if isinstance(args["data"], str) else type(args["data"]).__name__)
            check(data, name, kpt_shape) if kpt_shape is not None else check(data, name)
        device = select_device(args.get("device", ""))
        dtype = resolve_dtype(args.get("dtype"), bool(args.get("half", False)), self.model)
        if fp8_refused is None and dtype not in (torch.float32, torch.float16, torch.bfloat16):
            dtype = torch.float32
        elif fp8_refused is not None and dtype == H.FP8:
            raise NotImplementedError(f"val: {fp8_refused} is built for the 16-bit, split-float16 and fp32 storage types")
        was_training = self.model.training
        model = self.model.to(device)
        loader = TensorLoader({k: data[k] for k in keys}, int(args.get("batch") or 16), 0, 1, shuffle=False)
        try:
            self.metrics = (validator or default)(args)(model, loader, device, dtype)
        finally:
            model.train(was_training)
        self.predictor = None  # (the pass may have re-packed weights for another storage type)
        return self.metrics

    @staticmethod
    def _check_val_masks(data: dict, name: str) -> None:
        masks = data.get("masks")
        if masks is None:
            raise NotImplementedError("val: a segmentation model needs a dataset with 'masks' (the overlap index map (N, gh, gw) of every image); "
                                      f"data={name} has none")
        if not isinstance(masks, torch.Tensor) or masks.dim() != 3 or masks.shape[0] != data["img"].shape[0] or masks.dtype not in (torch.uint8, torch.int32):
            raise NotImplementedError("val: 'masks' must be the overlap index map, uint8 / int32 (N, gh, gw) with one map per image; one binary mask per "
                                      "label (overlap_mask=False) is not built")

    @staticmethod
    def _check_val_xywhr(data: dict, name: str) -> None:
        boxes = data["bboxes"]
        if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] != 5:
            shape = tuple(boxes.shape) if isinstance(boxes, torch.Tensor) else type(boxes).__name__
            raise NotImplementedError(f"val: an oriented-box model needs a dataset whose 'bboxes' are (M, 5) xywhr (normalised xywh and the angle in radians); "
                                      f"data={name} has {shape} (no angles)")

    @staticmethod
    def _check_val_keypoints(data: dict, name: str, kpt_shape) -> None:
        kpts = data.get("keypoints")
        nkpt, ndim = int(kpt_shape[0]), int(kpt_shape[1])
        takes = f"(M, {nkpt}, 3)" + (f" or (M, {nkpt}, 2)" if ndim == 2 else "")
        if kpts is None:
            raise NotImplementedError(f"val: a pose model needs a dataset with 'keypoints' {takes} (normalised x, y and the visibility of every label; dict / "
                                      f".pt) or 'synthetic-pose[:N]'; data={name} has none")
        ok = isinstance(kpts, torch.Tensor) and kpts.dim() == 3 and kpts.shape[0] == data["bboxes"].shape[0] and kpts.shape[1] == nkpt \
            and (kpts.shape[2] == 3 or (kpts.shape[2] == 2 and ndim == 2))
        if not ok:
            shape = tuple(kpts.shape) if isinstance(kpts, torch.Tensor) else type(kpts).__name__
            raise NotImplementedError(f"val: a pose model needs a dataset with 'keypoints' {takes}, one row per label, as the model's kpt_shape "
                                      f"{[nkpt, ndim]} asks; data={name} has {shape}")

    def fuse(self):
        self.model.fuse()
        return self

    def info(self, detailed: bool = False, verbose: bool = True):
        return self.model.info(detailed=detailed, verbose=verbose)

    @property
    def names(self):
        return self.model.names

    @property
    def device(self):
        return next(self.model.parameters()).device

    def to(self, device):
        self.model.to(device)
        return self


class YOLO(Model):
    """``YOLO(model, task=None, verbose=False)`` — reference models/yolo/model.py:11-23."""

    def __init__(self, model="yolov8s-p2-repvgg.yaml", task=None, verbose=False):
        super().__init__(model=model, task=task, verbose=verbose)
