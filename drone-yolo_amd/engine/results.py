"""Result containers (reference: ultralytics/engine/results.py: ``Results``, ``Boxes`` :1004, ``Keypoints`` :1320, ``OBB`` :1585).

Only the tensor-view surface the detection, segmentation, oriented-box and pose paths fill is kept (boxes, masks, obb, keypoints);
plotting / saving are out of scope.  ``Boxes`` wraps the (n, 6) rows [x1, y1, x2, y2, conf, cls]
that ``dy_nms`` + ``dy_scale_boxes`` produced on the device, ``Masks`` the (n, H, W) bytes of ``dy_process_mask``, ``OBB`` the (n, 7) rows
[x, y, w, h, rotation, conf, cls] of ``dy_nms_rotated`` + ``dy_scale_rboxes``, ``Keypoints`` the (n, nkpt, 2 | 3) rows of ``dy_kpt_decode`` +
``dy_scale_coords``.
"""
from __future__ import annotations

import numpy as np
import torch

from ..utils import ops


class BaseTensor:
    def __init__(self, data, orig_shape):
        self.data = data
        self.orig_shape = orig_shape

    @property
    def shape(self):
        return self.data.shape

    def cpu(self):
        return self if isinstance(self.data, np.ndarray) else self.__class__(self.data.cpu(), self.orig_shape)

    def numpy(self):
        return self if isinstance(self.data, np.ndarray) else self.__class__(self.data.cpu().numpy(), self.orig_shape)

    def cuda(self):
        return self.__class__(torch.as_tensor(self.data).cuda(), self.orig_shape)

    def to(self, *args, **kwargs):
        return self.__class__(torch.as_tensor(self.data).to(*args, **kwargs), self.orig_shape)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        return self.__class__(self.data[idx], self.orig_shape)


class Boxes(BaseTensor):
    """Detections of one image — reference results.py:1004-1170."""

    def __init__(self, boxes, orig_shape):
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        assert boxes.shape[-1] in {6, 7}, f"expected 6 or 7 values but got {boxes.shape[-1]}"
        super().__init__(boxes, orig_shape)
        self.is_track = boxes.shape[-1] == 7

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def id(self):
        return self.data[:, -3] if self.is_track else None

    @property
    def xywh(self):
        return ops.xyxy2xywh(self.xyxy)

    @property
    def xyxyn(self):
        xyxy = self.xyxy.clone() if isinstance(self.xyxy, torch.Tensor) else np.copy(self.xyxy)
        xyxy[..., [0, 2]] /= self.orig_shape[1]
        xyxy[..., [1, 3]] /= self.orig_shape[0]
        return xyxy

    @property
    def xywhn(self):
        xywh = ops.xyxy2xywh(self.xyxy)
        xywh[..., [0, 2]] /= self.orig_shape[1]
        xywh[..., [1, 3]] /= self.orig_shape[0]
        return xywh


class Masks(BaseTensor):
    """Instance masks of one image — reference results.py:1222-1280.  ``data``: (n, H, W) uint8, 0 / 1, on the device the pass ran on
    (the reference holds float 0.0 / 1.0 there; one byte per pixel is what ``dy_process_mask`` writes and a quarter of the memory).
    H x W is the input image (letterboxed size) or, with ``retina_masks``, the original image.  ``xy`` / ``xyn`` (polygon outlines) need
    ``cv2.findContours`` (ops.masks2segments, utils/ops.py:810-836), which this package does not depend on."""

    def __init__(self, masks, orig_shape):
        if masks.ndim == 2:
            masks = masks[None, :]
        super().__init__(masks, orig_shape)

    @property
    def xy(self):
        raise NotImplementedError("Masks.xy: polygon outlines need cv2.findContours, which this package does not depend on; use .data")

    @property
    def xyn(self):
        raise NotImplementedError("Masks.xyn: polygon outlines need cv2.findContours, which this package does not depend on; use .data")


class Keypoints(BaseTensor):
    """Keypoints of one image — reference results.py:1320-1440.  ``data``: (n, nkpt, 2) x, y or (n, nkpt, 3) x, y, visibility.  As in the
    reference, the x and y of a point whose visibility is below 0.5 are set to 0 (results.py:1373-1375); rows that come from the predictor
    have that done already by ``dy_scale_coords`` (``masked=True``)."""

    def __init__(self, keypoints, orig_shape, masked: bool = False):
        """``masked``: the rows already have the x and y of their invisible points at 0 (the predictor's, from ``dy_scale_coords``)."""
        if keypoints.ndim == 2:
            keypoints = keypoints[None, :]
        if keypoints.shape[2] == 3 and not masked:  # x, y, conf
            mask = keypoints[..., 2] < 0.5  # points with conf < 0.5 (not visible)
            if isinstance(keypoints, torch.Tensor) and keypoints.is_cuda:  # (no host round trip to ask whether any point is invisible)
                keypoints = torch.cat((torch.where(mask[..., None], torch.zeros_like(keypoints[..., :2]), keypoints[..., :2]), keypoints[..., 2:]), -1)
            elif bool(mask.any()):
                keypoints = keypoints.clone() if isinstance(keypoints, torch.Tensor) else np.copy(keypoints)
                keypoints[..., :2][mask] = 0
        super().__init__(keypoints, orig_shape)
        self.has_visible = self.data.shape[-1] == 3

    @property
    def xy(self):
        return self.data[..., :2]

    @property
    def xyn(self):
        xy = self.xy.clone() if isinstance(self.xy, torch.Tensor) else np.copy(self.xy)
        xy[..., 0] /= self.orig_shape[1]
        xy[..., 1] /= self.orig_shape[0]
        return xy

    @property
    def conf(self):
        return self.data[..., 2] if self.has_visible else None


class OBB(BaseTensor):
    """Oriented boxes of one image — reference results.py:1585-1806.  ``data``: (n, 7) [x, y, w, h, rotation, conf, cls], or (n, 8) with a
    track id in front of conf -- what ``YOLO.track`` leaves for an image whose tracker returned rows (``is_track``, ``id``)."""

    def __init__(self, boxes, orig_shape):
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        assert boxes.shape[-1] in {7, 8}, f"expected 7 or 8 values but got {boxes.shape[-1]}"
        super().__init__(boxes, orig_shape)
        self.is_track = boxes.shape[-1] == 8

    @property
    def xywhr(self):
        return self.data[:, :5]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def id(self):
        return self.data[:, -3] if self.is_track else None

    @property
    def xyxyxyxy(self):
        """(n, 4, 2) corner points."""
        return ops.xywhr2xyxyxyxy(self.xywhr)

    @property
    def xyxyxyxyn(self):
        """The corner points divided by the original image's width and height."""
        pts = self.xyxyxyxy
        pts = pts.clone() if isinstance(pts, torch.Tensor) else np.copy(pts)
        pts[..., 0] /= self.orig_shape[1]
        pts[..., 1] /= self.orig_shape[0]
        return pts

    @property
    def xyxy(self):
        """(n, 4) axis-aligned boxes around the corner points."""
        x, y = self.xyxyxyxy[..., 0], self.xyxyxyxy[..., 1]
        if isinstance(x, torch.Tensor):
            return torch.stack([x.amin(1), y.amin(1), x.amax(1), y.amax(1)], -1)
        return np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], -1)


class Results:
    """Per-image result — reference results.py (`Results`): orig_img, orig_shape, boxes, masks, obb, keypoints, names, path, speed.  An
    oriented-box result carries ``obb`` and no ``boxes``.  ``crop``: None, or — a result of ``predict(frames, crops=...)`` — the window of the
    frame the result was computed on, ``(frame, x0, y0, x1, y1)``; its boxes and keypoints are in frame pixels."""

    def __init__(self, orig_img, path, names, boxes=None, speed=None, orig_shape=None, masks=None, obb=None, keypoints=None):
        self._orig_img = orig_img
        self.orig_shape = tuple(orig_shape) if orig_shape is not None else tuple(orig_img.shape[:2])
        self.boxes = Boxes(boxes, self.orig_shape) if boxes is not None else None
        self.masks = Masks(masks, self.orig_shape) if masks is not None else None
        self.obb = OBB(obb, self.orig_shape) if obb is not None else None
        self.keypoints = (keypoints if isinstance(keypoints, Keypoints) else Keypoints(keypoints, self.orig_shape)) if keypoints is not None else None
        self.probs = None
        self.crop = None
        self.speed = speed if speed is not None else {"preprocess": None, "inference": None, "postprocess": None}
        self.names = names
        self.path = path

    @property
    def orig_img(self):
        """HWC uint8 image; for tensor sources converted lazily (reference ops.py:841-851 does it eagerly)."""
        im = self._orig_img
        if isinstance(im, torch.Tensor):
            im = (im.permute(1, 2, 0).contiguous() * 255).clamp(0, 255).to(torch.uint8).cpu().numpy()
            self._orig_img = im
        return im

    def __len__(self):
        for v in (self.boxes, self.masks, self.keypoints, self.obb):  # (the first that is there, as the reference's __len__)
            if v is not None:
                return len(v)
        return 0

    def cpu(self):
        r = Results(self._orig_img, self.path, self.names, None, self.speed, self.orig_shape)
        r.boxes = self.boxes.cpu() if self.boxes is not None else None
        r.masks = self.masks.cpu() if self.masks is not None else None
        r.obb = self.obb.cpu() if self.obb is not None else None
        r.keypoints = self.keypoints.cpu() if self.keypoints is not None else None
        r.crop = self.crop
        return r

    def numpy(self):
        r = Results(self._orig_img, self.path, self.names, None, self.speed, self.orig_shape)
        r.boxes = self.boxes.numpy() if self.boxes is not None else None
        r.masks = self.masks.numpy() if self.masks is not None else None
        r.obb = self.obb.numpy() if self.obb is not None else None
        r.keypoints = self.keypoints.numpy() if self.keypoints is not None else None
        r.crop = self.crop
        return r

    def to(self, *args, **kwargs):
        r = Results(self._orig_img, self.path, self.names, None, self.speed, self.orig_shape)
        r.boxes = self.boxes.to(*args, **kwargs) if self.boxes is not None else None
        r.masks = self.masks.to(*args, **kwargs) if self.masks is not None else None
        r.obb = self.obb.to(*args, **kwargs) if self.obb is not None else None
        r.keypoints = self.keypoints.to(*args, **kwargs) if self.keypoints is not None else None
        r.crop = self.crop
        return r

    def __getitem__(self, idx):
        r = Results(self._orig_img, self.path, self.names, None, self.speed, self.orig_shape)
        r.boxes = self.boxes[idx] if self.boxes is not None else None
        r.masks = self.masks[idx] if self.masks is not None else None
        r.obb = self.obb[idx] if self.obb is not None else None
        r.keypoints = self.keypoints[idx] if self.keypoints is not None else None
        r.crop = self.crop
        return r

    # ---- text forms of a detection result (reference results.py:633-666 verbose, :668-757 save_txt, :759-823 summary, :906-940 to_json) ----
    def verbose(self) -> str:
        """'2 persons, 1 car, ' — detections per class in ascending class order; '(no detections), ' for none."""
        if len(self) == 0:
            return "(no detections), "
        cls = torch.as_tensor((self.boxes if self.boxes is not None else self.obb).cls).cpu()
        out = ""
        for c in cls.unique():
            n = int((cls == c).sum())
            out += f"{n} {self.names[int(c)]}{'s' * (n > 1)}, "
        return out

    def summary(self, normalize: bool = False, decimals: int = 5) -> list:
        """One dict per detection: name, class, confidence, box {x1, y1, x2, y2} (divided by the image size with ``normalize``)."""
        if self.boxes is None:
            return []
        h, w = self.orig_shape if normalize else (1, 1)
        rows = torch.as_tensor(self.boxes.data).cpu().tolist()
        out = []
        for r in rows:
            k = int(r[-1])
            d = {"name": self.names[k], "class": k, "confidence": round(r[-2], decimals),
                 "box": {"x1": round(r[0] / w, decimals), "y1": round(r[1] / h, decimals), "x2": round(r[2] / w, decimals), "y2": round(r[3] / h, decimals)}}
            if self.boxes.is_track:
                d["track_id"] = int(r[-3])
            out.append(d)
        return out

    def to_json(self, normalize: bool = False, decimals: int = 5) -> str:
        import json

        return json.dumps(self.summary(normalize=normalize, decimals=decimals), indent=2)

    tojson = to_json

    def save_txt(self, txt_file, save_conf: bool = False) -> str:
        """Append one line per detection, `class x_center y_center width height [confidence]` with the box normalised to the image (the label format)."""
        from pathlib import Path

        lines = []
        if self.boxes is not None and len(self.boxes):
            xywhn = torch.as_tensor(self.boxes.xywhn).cpu().tolist()
            conf = torch.as_tensor(self.boxes.conf).cpu().tolist()
            cls = torch.as_tensor(self.boxes.cls).cpu().tolist()
            for b, s, c in zip(xywhn, conf, cls):
                vals = (int(c), *b) + ((s,) if save_conf else ())
                lines.append(("%g " * len(vals)).rstrip() % vals)
        if lines:
            Path(txt_file).parent.mkdir(parents=True, exist_ok=True)
            with open(txt_file, "a") as f:
                f.writelines(t + "\n" for t in lines)
        return str(txt_file)
