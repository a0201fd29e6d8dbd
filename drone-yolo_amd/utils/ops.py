"""Post-processing ops of the detection path (reference: ultralytics/utils/ops.py).

``non_max_suppression`` (:181-332) keeps the reference signature and return type; the work is
done by ``dy_nms`` (filter -> sort -> greedy suppression on the device), or with ``rotated=True`` by
``dy_nms_rotated`` (the same candidate stage, then ProbIoU fast NMS).  ``regularize_rboxes`` (:791-807),
``xywhr2xyxyxyxy`` (:572-600) and ``nms_rotated`` (:146-178) are the oriented-box helpers under the reference's names.  ``xywh2xyxy`` (:432-449),
``scale_boxes`` (:92-127), ``clip_boxes`` (:335-354), ``make_divisible`` (:130-143) and ``Profile``
(:17-62) are the small host helpers around it.
"""
from __future__ import annotations

import contextlib
import math
import time
from typing import List, Optional

import numpy as np
import torch

from .. import hip_ops as H


class Profile(contextlib.ContextDecorator):
    """Wall-clock timer that synchronises the device around the block — reference ops.py:17-62."""

    def __init__(self, t=0.0, device: Optional[torch.device] = None):
        self.t = t
        self.device = device
        self.cuda = bool(device and str(device).startswith("cuda"))

    def __enter__(self):
        self.start = self.time()
        return self

    def __exit__(self, type, value, traceback):
        self.dt = self.time() - self.start
        self.t += self.dt

    def __str__(self):
        return f"Elapsed time is {self.t} s"

    def time(self):
        if self.cuda:
            torch.cuda.synchronize(self.device)
        return time.perf_counter()


def make_divisible(x, divisor):
    """Nearest multiple of divisor not below x — reference ops.py:130-143."""
    if isinstance(divisor, torch.Tensor):
        divisor = int(divisor.max())
    return math.ceil(x / divisor) * divisor


def empty_like(x):
    return torch.empty_like(x, dtype=torch.float32) if isinstance(x, torch.Tensor) else np.empty_like(x, dtype=np.float32)


def xywh2xyxy(x):
    """(cx, cy, w, h) -> (x1, y1, x2, y2); output is always fp32 — reference ops.py:432-449."""
    assert x.shape[-1] == 4, f"input shape last dimension expected 4 but input shape is {x.shape}"
    y = empty_like(x)
    xy = x[..., :2]
    wh = x[..., 2:] / 2
    y[..., :2] = xy - wh
    y[..., 2:] = xy + wh
    return y


def xyxy2xywh(x):
    assert x.shape[-1] == 4, f"input shape last dimension expected 4 but input shape is {x.shape}"
    y = empty_like(x)
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def clip_boxes(boxes, shape):
    """Clamp xyxy boxes to (h, w) — reference ops.py:335-354."""
    if isinstance(boxes, torch.Tensor):
        boxes[..., 0] = boxes[..., 0].clamp(0, shape[1])
        boxes[..., 1] = boxes[..., 1].clamp(0, shape[0])
        boxes[..., 2] = boxes[..., 2].clamp(0, shape[1])
        boxes[..., 3] = boxes[..., 3].clamp(0, shape[0])
    else:
        boxes[..., [0, 2]] = boxes[..., [0, 2]].clip(0, shape[1])
        boxes[..., [1, 3]] = boxes[..., [1, 3]].clip(0, shape[0])
    return boxes


def letterbox_params(img1_shape, img0_shape, ratio_pad=None):
    """(gain, pad_x, pad_y) that undo a letterbox from img0 to img1 — the scalar part of ops.py:109-117."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1), round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1))
    else:
        gain, pad = ratio_pad[0][0], ratio_pad[1]
    return gain, pad[0], pad[1]


def scale_boxes(img1_shape, boxes, img0_shape, ratio_pad=None, padding=True, xywh=False):
    """Host/tensor helper with the reference semantics (ops.py:92-127); the predictor uses the
    fused device version ``dy_scale_boxes`` on the NMS output instead."""
    gain, px, py = letterbox_params(img1_shape, img0_shape, ratio_pad)
    if padding:
        boxes[..., 0] -= px
        boxes[..., 1] -= py
        if not xywh:
            boxes[..., 2] -= px
            boxes[..., 3] -= py
    boxes[..., :4] /= gain
    return clip_boxes(boxes, img0_shape)


def clip_coords(coords, shape):
    """Clip point coordinates (..., 2+) to the image (h, w) — reference ops.py:357-374."""
    if isinstance(coords, torch.Tensor):
        coords[..., 0] = coords[..., 0].clamp(0, shape[1])
        coords[..., 1] = coords[..., 1].clamp(0, shape[0])
    else:
        coords[..., 0] = coords[..., 0].clip(0, shape[1])
        coords[..., 1] = coords[..., 1].clip(0, shape[0])
    return coords


def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None, normalize=False, padding=True):
    """Rescale point coordinates (..., 2+) from img1_shape to img0_shape, in place — reference ops.py:756-788.  Unlike ``scale_boxes`` the
    pad is NOT rounded: (img1 - img0 * gain) / 2 as it comes.  The device form is ``dy_scale_coords``."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    if padding:
        coords[..., 0] -= pad[0]
        coords[..., 1] -= pad[1]
    coords[..., 0] /= gain
    coords[..., 1] /= gain
    coords = clip_coords(coords, img0_shape)
    if normalize:
        coords[..., 0] /= img0_shape[1]
        coords[..., 1] /= img0_shape[0]
    return coords


def regularize_rboxes(rboxes):
    """xywhr boxes with the angle brought into [0, pi/2): w and h swap where ``t % pi >= pi/2`` — reference ops.py:791-807."""
    x, y, w, h, t = rboxes.unbind(dim=-1)
    swap = t % math.pi >= math.pi / 2
    w_ = torch.where(swap, h, w)
    h_ = torch.where(swap, w, h)
    t = t % (math.pi / 2)
    return torch.stack([x, y, w_, h_, t], dim=-1)


def xywhr2xyxyxyxy(x):
    """(cx, cy, w, h, rotation) of shape (n, 5) or (b, n, 5) -> corner points (..., 4, 2), tensors or arrays — reference ops.py:572-600."""
    cos, sin, cat, stack = (torch.cos, torch.sin, torch.cat, torch.stack) if isinstance(x, torch.Tensor) else (np.cos, np.sin, np.concatenate, np.stack)
    ctr = x[..., :2]
    w, h, angle = (x[..., i : i + 1] for i in range(2, 5))
    cos_value, sin_value = cos(angle), sin(angle)
    vec1 = cat([w / 2 * cos_value, w / 2 * sin_value], -1)
    vec2 = cat([-h / 2 * sin_value, h / 2 * cos_value], -1)
    pt1 = ctr + vec1 + vec2
    pt2 = ctr + vec1 - vec2
    pt3 = ctr - vec1 - vec2
    pt4 = ctr - vec1 + vec2
    return stack([pt1, pt2, pt3, pt4], -2)


def nms_rotated(boxes, scores, threshold=0.45, use_triu=True):
    """Indices of the xywhr ``boxes`` (n, 5) that ProbIoU fast NMS keeps, in descending score order — reference ops.py:146-178, on the
    device through ``dy_nms_rotated``: the boxes become a one-class, one-image prediction whose class row holds the scores.
    Scores must lie in (0, 1]; ``use_triu`` selects an export form of the same result in the reference and is accepted and ignored."""
    H.require_device(boxes, "boxes")
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros((0,), dtype=torch.long, device=boxes.device)
    pred = torch.cat((boxes[:, :4].float().t(), scores.float()[None]), 0)[None].contiguous()
    theta = boxes[:, 4].float()[None].contiguous()
    bufs = H.nms_rotated(pred, theta, 0.0, float(threshold), max_det=min(n, 4096), max_nms=n, agnostic=True, nc=1)
    return bufs.index[0, : int(bufs.count[0])].long()


def non_max_suppression(
    prediction,
    conf_thres=0.25,
    iou_thres=0.45,
    classes=None,
    agnostic=False,
    multi_label=False,
    labels=(),
    max_det=300,
    nc=0,
    max_time_img=0.05,
    max_nms=30000,
    max_wh=7680,
    in_place=True,
    rotated=False,
    end2end=False,
    return_padded=False,
) -> List[torch.Tensor]:
    """Reference ops.py:181-332 on the device via ``dy_nms``: the predictor's single-label path and the validator's ``multi_label``
    path (one candidate per (anchor, class) pair above conf, ops.py:286-288; models/yolo/detect/val.py:93-106).

    ``rotated=True`` (ops.py:257-258, 307-309): ``prediction`` is (N, 4 + nc + 1, A) with the angle in the last row; the boxes stay xywh, the
    suppression is ``dy_nms_rotated``'s, the rows are (n_i, 7) [x, y, w, h, conf, cls, angle] and ``return_padded`` gives ``RNmsBuffers``
    (whose ``out`` columns are x, y, w, h, angle, conf, cls).  ``nc`` must be given, as the reference's predictor gives it: without it the
    reference counts the angle row as one more class AND reads it as the angle, which is not built; neither is ``multi_label``.

    Returns a list (one (n_i, 6) tensor [x1, y1, x2, y2, conf, cls] per image) like the reference;
    ``return_padded=True`` returns the device-resident ``NmsBuffers`` (out (N,max_det,6), count (N,),
    index (N,max_det)) without any host synchronisation.  ``max_time_img`` is accepted and ignored:
    the wall-clock break (ops.py:328-330) is non-deterministic and the device kernel has no need for it.
    """
    assert 0 <= conf_thres <= 1, f"Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0"
    assert 0 <= iou_thres <= 1, f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0"
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    if labels or end2end or prediction.shape[-1] == 6:
        raise NotImplementedError("labels (autolabelling) / end2end NMS variants are not on the accelerated path")
    if rotated and multi_label:
        raise NotImplementedError("multi_label NMS (the validator's) is not built for rotated boxes")
    if rotated and not nc:
        raise NotImplementedError("rotated NMS without nc (the reference then takes the angle row for a class as well) is not built: pass nc, the angle is the row behind the classes")
    H.require_device(prediction, "prediction")
    nc = nc or (prediction.shape[1] - 4)
    mask = None
    if classes is not None:
        mask = torch.zeros(nc, dtype=torch.uint8)
        mask[torch.as_tensor(list(classes), dtype=torch.long)] = 1
        mask = mask.to(prediction.device)
    if rotated:
        if prediction.shape[1] != 4 + nc + 1:
            raise ValueError(f"rotated NMS expects (N, 4 + nc + 1, A) with the angle in the last row, got {tuple(prediction.shape)}")
        rb = H.nms_rotated(prediction[:, : 4 + nc].float().contiguous(), prediction[:, -1].float().contiguous(), float(conf_thres), float(iou_thres),
                           max_det=int(max_det), max_nms=int(max_nms), max_wh=float(max_wh), agnostic=bool(agnostic), nc=int(nc), classes_mask=mask)
        if return_padded:
            return rb
        return [torch.cat((rb.out[i, :k, :4], rb.out[i, :k, 5:7], rb.out[i, :k, 4:5]), 1) for i, k in enumerate(rb.count.tolist())]
    pred = prediction if (prediction.dtype == torch.float32 and prediction.is_contiguous()) else prediction.float().contiguous()
    bufs = H.nms(pred, float(conf_thres), float(iou_thres), max_det=int(max_det), max_nms=int(max_nms),
                 max_wh=float(max_wh), agnostic=bool(agnostic), nc=int(nc), classes_mask=mask, multi_label=bool(multi_label))
    if return_padded:
        return bufs
    counts = bufs.count.tolist()  # one device->host sync for the whole batch
    return [bufs.out[i, :k].clone() for i, k in enumerate(counts)]
