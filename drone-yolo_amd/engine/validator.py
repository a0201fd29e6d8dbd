"""Validation step of the training loop on the device (reference: ultralytics/engine/validator.py ``BaseValidator.__call__`` :109-221
in its training branch, and models/yolo/detect/val.py ``DetectionValidator``: ``postprocess`` :93-106 = NMS with ``multi_label=True``
at conf 0.001, ``update_metrics`` :126-174, ``_process_batch`` :213-231, ``get_stats`` :181-190).

What runs where: the model pass (EMA weights, eval mode: BatchNorm folded, the trainer's storage type) and the validator's NMS
(``dy_nms`` with ``multi_label``: one candidate per (anchor, class) pair) on the device; AP on the host in numpy, as in the reference
(utils/metrics.py).  The matching of detections to labels runs on the device as well (``device_match``, on by default): ``dy_val_match`` matches every
batch on the padded NMS output behind the NMS, the statistics stay on the device for the whole set and come to the host once per
validation (``_collect_device``).  ``device_match=False`` is the reference's data flow, on the host image by image (``box_iou`` +
``match_predictions``, ``_collect_host``); the returned numbers are the same ("Validation matching on the device").
The validation loss is the criterion on Detect's raw maps of the same pass (validator.py:186-187).
Tensor datasets only (dataset files / augmentation are out of scope): ``data["val"]`` — a dict in the training set's
layout — or, when the dataset has no split, the training tensors themselves.

``DetectionValidator`` owns the call, both collect loops and the final assembly; a task differs in its class data (``stat_keys``,
``metrics_cls``, ``val_loss``) and four hooks: ``_nms`` (the task's half of the pass), ``_labels``, ``_match_device`` and ``_match_host``.
``SegmentationValidator`` (models/yolo/segment/val.py) adds the mask statistics of a segmentation model: ``dy_val_mask_match`` behind the box
matching, or the reference's mask branch on the host ("Segmentation validation").
``OBBValidator`` (models/yolo/obb/val.py) scores an oriented-box model: ``dy_nms_rotated_ml`` and ``dy_val_match_rotated`` (ProbIoU), or the
reference's data flow on the host ("Oriented-box validation").
``PoseValidator`` (models/yolo/pose/val.py) adds the keypoint statistics of a pose model: ``dy_val_oks_match`` (object keypoint similarity) behind
the box matching, or the reference's keypoint branch on the host ("Pose validation")."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from .. import hip_ops as H
from ..utils import ops
from ..utils.metrics import OKS_SIGMA, DetMetrics, OBBMetrics, PoseMetrics, SegmentMetrics, batch_probiou, box_iou, kpt_iou, mask_iou, match_predictions


class DetectionValidator:
    stat_keys = ("tp",)  # what the matchers return, per detection; conf, pred_cls and target_cls follow in ``stats``
    metrics_cls = DetMetrics
    val_loss = True  # the criterion on the raw maps of the same pass: ``val/*_loss`` in the dict

    def __init__(self, args: Optional[dict] = None):
        a = dict(conf=None, iou=0.7, max_det=300, single_cls=False, agnostic_nms=False, device_match=True)
        a.update({k: v for k, v in (args or {}).items() if k in a})
        self.conf = 0.001 if a["conf"] is None else float(a["conf"])  # default 0.001 in val mode (validator.py:134)
        self.iou, self.max_det = float(a["iou"]), int(a["max_det"])
        self.agnostic = bool(a["single_cls"] or a["agnostic_nms"])
        self.single_cls = bool(a["single_cls"])
        self.device_match = bool(a["device_match"])  # package extension (cfg/default.yaml): matching through dy_val_match
        self.iouv = np.linspace(0.5, 0.95, 10)  # detect/val.py:37
        self.metrics = self.metrics_cls()
        self.last_stats = None  # what the last call gathered (per-image lists on the host path, one block on the device path)
        self.last_counts = None  # and the kept rows of every image, int32

    def __call__(self, model, loader, device, dtype: torch.dtype) -> Dict[str, float]:
        """``model``: the model carrying the weights to evaluate (the trainer loads the EMA copy), put in eval mode here and
        left there; ``loader``: batches in the training layout (uint8 images + normalised xywh labels).  Returns the reference's
        ``results_dict`` (+ ``val/*_loss`` with ``val_loss``) + ``fitness``, rounded to 5 digits (validator.py:204-207)."""
        model.eval()
        nc = model.yaml["nc"]
        stats = {k: [] for k in (*self.stat_keys, "conf", "pred_cls", "target_cls")}
        loss = torch.zeros(3, device=device) if self.val_loss else None
        if self.val_loss and getattr(model, "criterion", None) is None:
            model.criterion = model.init_criterion()
        det = model.model[-1]
        fuse_tail = getattr(det, "fuse_tail", False)
        try:
            nb = (self._collect_device if self.device_match else self._collect_host)(model, loader, device, dtype, nc, stats, loss, det)
        finally:
            det.fuse_tail = fuse_tail  # (a predictor that shares the model keeps its fused tail: ADVICE r4)
        self.last_stats = stats
        out = {k: 0.0 for k in self.metrics_cls.keys + ("fitness",)}
        if stats["tp"]:
            cat = {k: np.concatenate(v, 0) for k, v in stats.items()}
            if len(cat["target_cls"]):
                self.metrics.process(*cat.values())
                out = self.metrics.results_dict
        if self.val_loss:
            vl = (loss / max(nb, 1)).cpu().tolist()
            out.update({"val/box_loss": vl[0], "val/cls_loss": vl[1], "val/dfl_loss": vl[2]})
        return {k: round(float(v), 5) for k, v in out.items()}

    # ---- the task's hooks ----------------------------------------------------------------------------------------------------
    def _nms(self, y, aux, nc, batch):
        """The task's half of the pass: the head's outputs -> the padded NMS buffers and the tensors the matchers need besides."""
        return ops.non_max_suppression(y, self.conf, self.iou, nc=nc, multi_label=True, agnostic=self.agnostic, max_det=self.max_det, return_padded=True), ()

    def _labels(self, bboxes: torch.Tensor, w: int, h: int, lim: torch.Tensor) -> torch.Tensor:
        """_prepare_batch (detect/val.py:108-117) on normalised xywh labels: xyxy in pixels, then ops.scale_boxes to the original image — for a
        tensor dataset gain 1, pad 0 and the clip to the image (ops.py:92-127, 335-354).  Elementwise fp32 torch operations: the same bits
        wherever ``bboxes`` lives.  ``lim``: fp32 (w, h, w, h) on the same device."""
        return torch.minimum((ops.xywh2xyxy(bboxes.float()) * lim).clamp_min(0), lim)

    def _match_device(self, bufs, tbox, cls, bi, wh, extras) -> Dict[str, torch.Tensor]:
        return dict(tp=H.val_match(bufs, tbox, cls, bi, self.iouv, wh, single_cls=self.single_cls))  # (new tensors on every call)

    def _match_host(self, pn: np.ndarray, tbox: np.ndarray, cls: np.ndarray, wh, extras, si: int) -> Dict[str, np.ndarray]:
        """One image with labels and rows: ``pn`` as ``_clipped`` leaves them."""
        return dict(tp=match_predictions(pn[:, 5], cls, box_iou(tbox, pn[:, :4]), self.iouv))

    # ---- the pass and the two loops ------------------------------------------------------------------------------------------
    def _pass(self, model, batch, device, dtype, nc, det, loss):
        img = batch["img"].to(device)
        x = (img.float() / 255.0) if img.dtype == torch.uint8 else img.float()  # detect/val.py:49-52
        with torch.no_grad():
            det.fuse_tail = False  # the head returns (y, aux) with its raw maps: Detect's feats, Segment's (feats, mc, p), OBB's (feats, angle)
            y, aux = model._predict_once(x.contiguous(), image_dtype=dtype)
            if self.val_loss:
                loss += model.criterion(aux, batch)[1]  # validator.py:186-187: loss items of the same pass
            bufs, extras = self._nms(y, aux, nc, batch)
        return img.shape, bufs, extras

    def _clipped(self, rows: np.ndarray, w: int, h: int) -> np.ndarray:
        """_prepare_pred (detect/val.py:119-124): ops.scale_boxes at gain 1, pad 0 is the clip, columns 0 and 2 to [0, w], 1 and 3 to [0, h]
        (of an xywh row the width and height too); class 0 with ``single_cls``."""
        pn = rows.copy()
        pn[:, [0, 2]] = pn[:, [0, 2]].clip(0, w)
        pn[:, [1, 3]] = pn[:, [1, 3]].clip(0, h)
        if self.single_cls:
            pn[:, -1] = 0
        return pn

    def _collect_device(self, model, loader, device, dtype, nc, stats, loss, det) -> int:
        """``device_match``: fills ``stats`` with what ``_collect_host`` gathers (image order, then row order), matched on the device.
        Nothing in the loop waits for the device; the accumulated tensors go to the host once each after it."""
        nb = n_img = 0
        rows, counts, tcls, timg = [], [], [], []
        tps = {k: [] for k in self.stat_keys}
        lim = {}
        for batch in loader:
            nb += 1
            (b, _, h, w), bufs, extras = self._pass(model, batch, device, dtype, nc, det, loss)
            if (w, h) not in lim:
                lim[(w, h)] = torch.tensor((w, h, w, h), dtype=torch.float32, device=device)
            cls = batch["cls"].to(device).view(-1).float()
            bi = batch["batch_idx"].to(device).view(-1).to(torch.int32)
            tbox = self._labels(batch["bboxes"].to(device), w, h, lim[(w, h)])
            for k, v in self._match_device(bufs, tbox, cls, bi, (w, h), extras).items():
                tps[k].append(v)
            rows.append(bufs.out[..., bufs.ROW - 2 :].clone()), counts.append(bufs.count.clone())  # (the NMS buffers may be reused by the next batch)
            tcls.append(cls), timg.append(bi + n_img)
            n_img += b
        if nb == 0:
            return nb
        rows, counts = torch.cat(rows).cpu().numpy(), torch.cat(counts).cpu().numpy()
        tps = {k: torch.cat(v).cpu().numpy() for k, v in tps.items()}
        tcls, timg = torch.cat(tcls).cpu().numpy(), torch.cat(timg).cpu().numpy().astype(np.int64)
        keep = np.arange(self.max_det)[None, :] < counts[:, None]
        conf, pred_cls = rows[keep][:, 0], rows[keep][:, 1]
        if self.single_cls:
            pred_cls = np.zeros_like(pred_cls)
        # an image without predictions but with labels adds float64 zeros(0) on the host path, which makes its concatenated conf / pred_cls
        # float64: the same type here, so that AP's argsort sees the same array
        if bool(((counts == 0) & (np.bincount(timg, minlength=len(counts))[: len(counts)] > 0)).any()):
            conf, pred_cls = conf.astype(np.float64), pred_cls.astype(np.float64)
        if len(conf) or len(tcls):
            for k, v in tps.items():
                stats[k].append(v[keep].astype(bool))
            stats["conf"].append(conf), stats["pred_cls"].append(pred_cls)
            stats["target_cls"].append(tcls[np.argsort(timg, kind="stable")])
        self.last_counts = counts
        return nb

    def _collect_host(self, model, loader, device, dtype, nc, stats, loss, det) -> int:
        """``device_match=False``: detect/val.py:126-174 image by image on CPU arrays; one read-back of the counts and the rows per batch."""
        nb = 0
        all_counts = []
        for batch in loader:
            nb += 1
            (_, _, h, w), bufs, extras = self._pass(model, batch, device, dtype, nc, det, loss)
            counts = bufs.count.cpu().tolist()
            out = bufs.out.cpu()
            extras = tuple(t.cpu() for t in extras)
            bi = batch["batch_idx"].long().cpu()
            all_counts += counts
            lim = torch.tensor((w, h, w, h), dtype=torch.float32)
            for si, k in enumerate(counts):
                sel = bi == si
                cls = batch["cls"].cpu()[sel].view(-1).numpy()
                tps = {key: np.zeros((k, len(self.iouv)), dtype=bool) for key in self.stat_keys}
                if k == 0:
                    if len(cls):
                        for key, v in tps.items():
                            stats[key].append(v)
                        stats["conf"].append(np.zeros(0)), stats["pred_cls"].append(np.zeros(0)), stats["target_cls"].append(cls)
                    continue
                pn = self._clipped(out[si, :k].numpy(), w, h)
                if len(cls):
                    tbox = self._labels(batch["bboxes"].cpu()[sel], w, h, lim).numpy()  # (a dataset held on the device: host arithmetic)
                    tps = self._match_host(pn, tbox, cls, (w, h), extras, si)
                for key in self.stat_keys:
                    stats[key].append(tps[key])
                stats["conf"].append(pn[:, -2]), stats["pred_cls"].append(pn[:, -1]), stats["target_cls"].append(cls)
        self.last_counts = np.array(all_counts, dtype=np.int32)
        return nb


# ---- segmentation: the reference's mask branch on the host (models/yolo/segment/val.py), piece by piece --------------------------------
def host_pred_masks(proto: torch.Tensor, coef: torch.Tensor, boxes: torch.Tensor, in_hw) -> torch.Tensor:
    """``ops.process_mask(proto, coef, boxes, shape=in_hw)`` with ``upsample=False`` (utils/ops.py:679-709) on CPU fp32 tensors: proto
    (nm, mh, mw), coef (n, nm), boxes (n, 4) unscaled xyxy in input pixels -> float 0 / 1 masks (n, mh, mw) at PROTOTYPE resolution."""
    c, mh, mw = proto.shape
    ih, iw = in_hw
    masks = (coef.float() @ proto.float().reshape(c, -1)).view(-1, mh, mw)
    b = boxes.float().clone()
    b[:, 0] *= mw / iw
    b[:, 2] *= mw / iw
    b[:, 3] *= mh / ih
    b[:, 1] *= mh / ih
    x1, y1, x2, y2 = torch.chunk(b[:, :, None], 4, 1)  # crop_mask (ops.py:660-676)
    r = torch.arange(mw, dtype=x1.dtype)[None, None, :]
    cc = torch.arange(mh, dtype=x1.dtype)[None, :, None]
    return (masks * ((r >= x1) * (r < x2) * (cc >= y1) * (cc < y2))).gt_(0.0)


def host_gt_masks(label_map: torch.Tensor, nl: int, proto_hw) -> torch.Tensor:
    """The overlap label map (gh, gw) of one image -> one float 0 / 1 mask per label (nl, mh, mw): ``gt == index`` and, when the sizes differ,
    ``F.interpolate(bilinear, align_corners=False)`` + ``gt_(0.5)`` (segment/val.py:196-203)."""
    index = torch.arange(nl).view(nl, 1, 1) + 1
    gt = torch.where(label_map[None].long().repeat(nl, 1, 1) == index, 1.0, 0.0)
    if tuple(gt.shape[1:]) != tuple(proto_hw):
        gt = F.interpolate(gt[None], tuple(proto_hw), mode="bilinear", align_corners=False)[0]
        gt = gt.gt_(0.5)
    return gt


def host_mask_iou(gt: torch.Tensor, pred: torch.Tensor) -> np.ndarray:
    """``mask_iou`` on the flattened masks: (nl, n) fp32."""
    px = int(np.prod(gt.shape[1:]))
    return mask_iou(gt.reshape(gt.shape[0], px).numpy(), pred.reshape(pred.shape[0], px).numpy())


def check_mask_grids(proto_hw, map_hw) -> int:
    """The two grid relations that occur: the label map on the prototype grid (ratio 1), or the prototype grid exactly twice the map on both
    axes (ratio 2: the P2 models).  Anything else is refused."""
    (mh, mw), (gh, gw) = (int(v) for v in proto_hw), (int(v) for v in map_hw)
    if (mh, mw) == (gh, gw):
        return 1
    if (mh, mw) == (2 * gh, 2 * gw):
        return 2
    raise ValueError(f"segmentation val: the prototype grid {mh} x {mw} must equal the label map's {gh} x {gw} or be exactly twice it on both axes")


class SegmentationValidator(DetectionValidator):
    """``SegmentationValidator`` of the reference (models/yolo/segment/val.py): ``DetectionValidator`` plus the mask statistics ``tp_m``.
    The model pass, the ``multi_label`` NMS (``nc=`` given: the 32 coefficient channels ride behind the classes), ``dy_mask_gather`` and the
    box matching run as in the detection validator; with ``device_match`` the masks are scored by ``dy_val_mask_match`` on the prototypes
    (no mask is stored, nothing in the batch loop waits for the device), without it by the reference's data flow on the host, image by
    image (``host_pred_masks`` / ``host_gt_masks`` / ``host_mask_iou`` / ``match_predictions``).  The dataset carries ``masks``: the
    reference's ``overlap_mask=True`` index map (N, gh, gw).  No validation loss (in eval mode the head hands on concatenated coefficients, ``v8SegmentationLoss``
    takes the per-level maps; the reference's stand-alone ``val`` computes none): the dict holds the eight metrics and ``fitness``.  The trainer
    calls this validator per epoch for a ``SegmentationModel`` whose validation split carries ``masks`` (engine/trainer.py)."""

    stat_keys = ("tp", "tp_m")
    metrics_cls = SegmentMetrics
    val_loss = False

    @staticmethod
    def _label_cap(loader) -> int:
        """The largest label count of one image over the whole set: one read before the loop (it sizes the kernel's per-label outputs)."""
        bi = loader.d["batch_idx"].reshape(-1).long()
        if not bi.numel():
            return 1
        per = torch.zeros(int(loader.n), dtype=torch.long, device=bi.device).index_add_(0, bi, torch.ones_like(bi))
        return max(int(per.max()), 1)

    def _collect_device(self, model, loader, *rest) -> int:
        self._l_cap = self._label_cap(loader)
        return super()._collect_device(model, loader, *rest)

    def _nms(self, y, aux, nc, batch):
        if not (isinstance(aux, tuple) and len(aux) == 3):  # Segment returns (cat([y, mc]), (feats, mc, p))
            raise RuntimeError("SegmentationValidator needs a model whose head is Segment")
        y = y.float().contiguous()
        bufs, _ = super()._nms(y, aux, nc, batch)
        side, protos, masks = H.mask_gather(bufs, pred=y, nc=nc), aux[2], batch["masks"]
        check_mask_grids(protos.shape[2:], masks.shape[1:])
        return bufs, (side, protos, masks)

    def _match_device(self, bufs, tbox, cls, bi, wh, extras) -> Dict[str, torch.Tensor]:
        side, protos, masks = extras
        tpm = H.val_mask_match(bufs, protos, side, masks.to(bufs.out.device), cls, bi, self.iouv, wh, self._l_cap, single_cls=self.single_cls)
        return dict(super()._match_device(bufs, tbox, cls, bi, wh, extras), tp_m=tpm)

    def _match_host(self, pn, tbox, cls, wh, extras, si) -> Dict[str, np.ndarray]:  # segment/val.py:90-133
        side, protos, gmaps = extras
        k = len(pn)
        pm = host_pred_masks(protos[si], side[si, :k, 4:], side[si, :k, :4], (wh[1], wh[0]))  # (the UNSCALED, unclipped NMS boxes)
        gt = host_gt_masks(gmaps[si], len(cls), protos.shape[2:])
        return dict(super()._match_host(pn, tbox, cls, wh, extras, si), tp_m=match_predictions(pn[:, 5], cls, host_mask_iou(gt, pm), self.iouv))


# ---- oriented boxes (models/yolo/obb/val.py) ---------------------------------------------------------------------------------------------
def obb_labels(bboxes: torch.Tensor, w: int, h: int, lim: torch.Tensor) -> torch.Tensor:
    """``OBBValidator._prepare_batch`` on the (L, 5) normalised xywhr labels of a batch: ``bboxes[:, :4] * (w, h, w, h)``, then
    ``scale_boxes(xywh=True)`` at gain 1 / pad 0, which leaves ``clip_boxes`` (columns 0 and 2 to [0, w], 1 and 3 to [0, h]: the width and
    height too).  The angle is untouched.  Elementwise fp32 torch operations: the same bits wherever ``bboxes`` lives.  ``lim``: fp32
    (w, h, w, h) on the same device."""
    t = bboxes.float().clone()
    t[:, :4] = torch.minimum((t[:, :4] * lim).clamp_min(0), lim)
    return t


class OBBValidator(DetectionValidator):
    """``OBBValidator`` of the reference (models/yolo/obb/val.py): ``DetectionValidator`` whose NMS is the rotated ``multi_label`` one
    (``dy_nms_rotated_ml``: ProbIoU fast NMS over every (anchor, class) pair above conf) and whose matching is ``match_predictions`` on
    ``batch_probiou(gt, det)``.  With ``device_match`` a batch is matched by ``dy_val_match_rotated`` behind the NMS and nothing in the batch
    loop waits for the device; without it the matching is the reference's data flow on the host, image by image.  The dataset's ``bboxes``
    are (M, 5) normalised xywh + the angle in radians.  No validation loss (in eval mode the head hands on the angle, ``v8OBBLoss`` takes its
    logit; the reference's stand-alone ``val`` computes none): the dict holds the four metrics and ``fitness``.  The trainer calls this
    validator per epoch for an ``OBBModel`` (engine/trainer.py)."""

    metrics_cls = OBBMetrics
    val_loss = False
    _labels = staticmethod(obb_labels)

    def _nms(self, y, aux, nc, batch):
        if not (isinstance(aux, tuple) and len(aux) == 2) or y.shape[1] != 4 + nc + 1:  # OBB returns (cat([y, angle], 1), (feats, angle))
            raise RuntimeError("OBBValidator needs a model whose head is OBB")
        y = y.float()
        return H.nms_rotated_ml(y[:, : 4 + nc].contiguous(), y[:, -1].contiguous(), self.conf, self.iou, max_det=self.max_det, agnostic=self.agnostic, nc=nc), ()

    def _match_device(self, bufs, tbox, cls, bi, wh, extras) -> Dict[str, torch.Tensor]:
        return dict(tp=H.val_match_rotated(bufs, tbox, cls, bi, self.iouv, wh, single_cls=self.single_cls))  # (new tensors on every call)

    def _match_host(self, pn, tbox, cls, wh, extras, si) -> Dict[str, np.ndarray]:
        iou = batch_probiou(torch.from_numpy(np.ascontiguousarray(tbox, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(pn[:, :5]))).numpy()
        return dict(tp=match_predictions(pn[:, 6], cls, iou, self.iouv))

    def host_match(self, rows: np.ndarray, tbox: np.ndarray, cls: np.ndarray, w: int, h: int) -> np.ndarray:
        """``_prepare_pred`` + ``_process_batch`` of one image on the host: ``rows`` (k, 7) = x, y, w, h, theta, conf, cls as the NMS left
        them, ``tbox`` (L, 5) prepared labels, ``cls`` (L,) -> tp (k, len(iouv)) bool."""
        if not len(cls) or not len(rows):
            return np.zeros((len(rows), len(self.iouv)), dtype=bool)
        return self._match_host(self._clipped(rows, w, h), tbox, cls, (w, h), (), 0)["tp"]


# ---- pose (models/yolo/pose/val.py) ------------------------------------------------------------------------------------------------------
def pose_label_kpts(kpts: torch.Tensor, w: int, h: int, lim: torch.Tensor) -> torch.Tensor:
    """``PoseValidator._prepare_batch`` on the (L, nkpt, 2 | 3) normalised label keypoints of a batch: ``x * w``, ``y * h``, then
    ``scale_coords`` at gain 1 / pad 0, which leaves ``clip_coords`` (x to [0, w], y to [0, h]); the visibility is untouched, and a set without
    one (ndim 2) gets the all-visible column the reference's dataset appends.  Returns (L, nkpt, 3).  Elementwise fp32 torch operations: the
    same bits wherever ``kpts`` lives.  ``lim``: fp32 (w, h, w, h) on the same device."""
    t = kpts.float()
    xy = torch.minimum((t[..., :2] * lim[:2]).clamp_min(0), lim[:2])
    vis = t[..., 2:3] if t.shape[-1] == 3 else torch.ones_like(xy[..., :1])
    return torch.cat((xy, vis), -1)


class PoseValidator(DetectionValidator):
    """``PoseValidator`` of the reference (models/yolo/pose/val.py): ``DetectionValidator`` plus the keypoint statistics ``tp_p``:
    ``match_predictions`` on ``kpt_iou(gt_kpts, pred_kpts, sigma, area = box area * 0.53)``.  The model pass, the ``multi_label`` NMS (``nc=``
    given: the keypoint channels ride behind the classes) and the box matching run as in the detection validator; with ``device_match`` the
    keypoints are scored by ``dy_val_oks_match``, which reads the kept anchors' keypoints out of the head's (N, 4 + nc + nk, A) tensor through the
    NMS's index (no gather launch, nothing in the batch loop waits for the device), without it by the reference's data flow on the host, image
    by image.  The dataset carries ``keypoints`` (M, nkpt, 3): normalised x, y and the visibility.  ``sigma``: the COCO constants for
    ``kpt_shape == [17, 3]``, ``ones(nkpt) / nkpt`` otherwise.  No validation loss (``v8PoseLoss`` is not built): the dict holds the eight
    metrics and ``fitness``."""

    stat_keys = ("tp", "tp_p")
    metrics_cls = PoseMetrics
    val_loss = False

    def __call__(self, model, loader, device, dtype: torch.dtype) -> Dict[str, float]:
        head = model.model[-1]
        if getattr(head, "kpt_shape", None) is None:
            raise RuntimeError("PoseValidator needs a model whose head is Pose")
        self.kpt_shape = tuple(int(v) for v in head.kpt_shape)
        self.sigma = OKS_SIGMA if list(self.kpt_shape) == [17, 3] else np.ones(self.kpt_shape[0]) / self.kpt_shape[0]
        self._lim = {}  # (w, h) -> the fp32 (w, h, w, h) of pose_label_kpts on the device: one upload per image size
        return super().__call__(model, loader, device, dtype)

    def _nms(self, y, aux, nc, batch):
        nk = self.kpt_shape[0] * self.kpt_shape[1]
        if not (isinstance(aux, tuple) and len(aux) == 2) or y.dim() != 3 or y.shape[1] != 4 + nc + nk:  # Pose returns (cat([y, pred_kpt], 1), (feats, kpt))
            raise RuntimeError("PoseValidator needs a model whose head is Pose")
        y = y.float().contiguous()
        bufs, _ = super()._nms(y, aux, nc, batch)
        self._nc = nc
        return bufs, (y, batch["keypoints"], batch["batch_idx"], bufs.index)

    def _match_device(self, bufs, tbox, cls, bi, wh, extras) -> Dict[str, torch.Tensor]:
        y, kpts = extras[0], extras[1].to(bufs.out.device)
        if tuple(wh) not in self._lim:
            self._lim[tuple(wh)] = torch.tensor((wh[0], wh[1], wh[0], wh[1]), dtype=torch.float32, device=kpts.device)
        lim = self._lim[tuple(wh)]
        tpp = H.val_oks_match(bufs, y, self.kpt_shape, tbox, pose_label_kpts(kpts, wh[0], wh[1], lim), cls, bi, self.sigma, self.iouv, wh,
                              nc=self._nc, single_cls=self.single_cls)
        return dict(super()._match_device(bufs, tbox, cls, bi, wh, extras), tp_p=tpp)

    def _match_host(self, pn, tbox, cls, wh, extras, si) -> Dict[str, np.ndarray]:  # pose/val.py:73-91, 146-184
        y, kpts, bi, index = extras
        (w, h), k = wh, len(pn)
        nkpt, ndim = self.kpt_shape
        pk = y[si][4 + self._nc :, index[si, :k].long()].t().reshape(k, nkpt, ndim).clone()  # the kept anchors' keypoint channels, as the NMS rows carry them
        pk[..., 0].clamp_(0, w)  # ops.scale_coords at gain 1 / pad 0: clip_coords
        pk[..., 1].clamp_(0, h)
        gt = pose_label_kpts(kpts[bi.long() == si], w, h, torch.tensor((w, h, w, h), dtype=torch.float32))
        tb = torch.from_numpy(np.ascontiguousarray(tbox, dtype=np.float32))
        area = ((tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])) * 0.53  # ops.xyxy2xywh(gt_bboxes)[:, 2:].prod(1) * 0.53
        oks = kpt_iou(gt, pk, area, self.sigma).numpy()
        return dict(super()._match_host(pn, tbox, cls, wh, extras, si), tp_p=match_predictions(pn[:, 5], cls, oks, self.iouv))
