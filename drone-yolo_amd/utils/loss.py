"""Detection training loss on the device (reference: ultralytics/utils/loss.py:157-260 ``v8DetectionLoss``).

TaskAlignedAssigner + BCE / CIoU / DFL, value and gradient, through ``dy_detection_loss``.  When the head maps carry an
autograd graph (training forward) the returned loss is differentiable: ``loss.backward()`` feeds the kernel's gradient
w.r.t. the head outputs into the backward of the model (nn/autograd_ops.py)."""
from __future__ import annotations

import numpy as np
import torch

from .. import hip_ops as H


class v8DetectionLoss:
    """Same constructor idea and call contract as the reference: ``loss, loss_items = criterion(preds, batch)``."""

    width = 5  # columns of the label table ``targets_to_gt`` builds and ``from_gt`` takes (the trainer sizes its static table by it)

    def __init__(self, model, tal_topk: int = 10, box: float = 7.5, cls: float = 0.5, dfl: float = 1.5):
        m = model.model[-1]  # Detect()
        h = getattr(model, "args", None)
        self.box, self.cls, self.dfl = (getattr(h, "box", box), getattr(h, "cls", cls), getattr(h, "dfl", dfl)) if h else (box, cls, dfl)
        self.stride, self.nc, self.reg_max, self.no = m.stride, m.nc, m.reg_max, m.nc + m.reg_max * 4
        self.topk = tal_topk

    @staticmethod
    def preprocess(targets: torch.Tensor, batch_size: int, scale_tensor: torch.Tensor) -> torch.Tensor:
        """(N, 6) [image, cls, x, y, w, h normalised] -> (B, n_max, 5) [cls, x1, y1, x2, y2] pixels — loss.py:180-195.
        Vectorised on the host (labels arrive on the host from the loader; one scatter instead of the reference's per-image loop,
        no device synchronisation).  numpy, not torch: a torch CPU op above the intra-op grain wakes the whole OpenMP pool, which on
        a GPU box is sized by the HOST's core count while the process owns a 16-core CFS quota — the pool's spin-waits spend the
        quota and the kernel parks every thread of the process until the next 100 ms period (r05: one such stall per 30-60 training
        steps, each longer than the ~3 steps of work the launch queue holds)."""
        t = targets.detach().cpu().float().numpy()
        nl, ne = t.shape
        if nl == 0:
            return torch.zeros(batch_size, 0, ne - 1)
        img = t[:, 0].astype(np.int64)
        counts = np.bincount(img, minlength=batch_size)
        order = np.argsort(img, kind="stable")
        start = np.cumsum(counts) - counts
        pos = np.arange(nl) - start[img[order]]  # rank of each label inside its image, in the order the labels came
        out = np.zeros((batch_size, int(counts.max()), ne - 1), dtype=np.float32)
        out[img[order], pos] = t[order, 1:]
        sc = scale_tensor.detach().cpu().float().numpy()
        xy, half = out[..., 1:3] * sc[:2], out[..., 3:5] * sc[2:] / np.float32(2)  # xywh2xyxy (utils/ops.py:432-449) in fp32, as torch computes it
        out[..., 1:3], out[..., 3:5] = xy - half, xy + half
        return torch.from_numpy(out)

    @staticmethod
    def check_classes(gt: torch.Tensor, nc: int) -> None:
        """Refuse a HOST box table with a class outside [0, nc) before any launch: the kernels index the class logits of a row with it
        unchecked.  A device table is the caller's (a graph-replayed trainer fills it from a table that went through here)."""
        if gt.is_cuda or gt.numel() == 0:
            return
        c = gt.detach()[..., 0].float().numpy()
        ok = (c >= 0) & (c < nc) & (c == np.floor(c))  # NaN fails every comparison
        if not ok.all():
            bad = c[~ok]
            raise ValueError(f"detection loss: {bad.size} label(s) with a class outside [0, {nc}), e.g. {bad.flat[0]!r}")

    def targets_to_gt(self, batch, batch_size: int, img_hw) -> torch.Tensor:
        """The batch's labels as the (B, n_max, 5) pixel-box table on the host (``preprocess``); img_hw = (h, w) of the images."""
        imgsz = torch.tensor([float(img_hw[1]), float(img_hw[0]), float(img_hw[1]), float(img_hw[0])], dtype=torch.float32)
        targets = torch.cat((batch["batch_idx"].view(-1, 1).float().cpu(), batch["cls"].view(-1, 1).float().cpu(),
                             batch["bboxes"].float().cpu()), 1)
        gt = self.preprocess(targets, batch_size, imgsz)
        self.check_classes(gt, self.nc)
        return gt

    def __call__(self, preds, batch):
        feats = preds[1] if isinstance(preds, tuple) else preds
        hw = (feats[0].shape[2] * float(self.stride[0]), feats[0].shape[3] * float(self.stride[0]))
        return self.from_gt(preds, self.targets_to_gt(batch, feats[0].shape[0], hw))

    def from_gt(self, preds, gt: torch.Tensor):
        """loss, loss_items from the box table itself (host or device, zero rows = padding): what ``__call__`` does after
        ``preprocess``.  A trainer that replays the step as a hipGraph keeps ``gt`` in a static device buffer."""
        feats = preds[1] if isinstance(preds, tuple) else preds
        self.check_classes(gt, self.nc)
        strides = [float(s) for s in self.stride]
        if any(f.requires_grad for f in feats):
            if self.topk != 10:
                raise NotImplementedError("the differentiable path uses the default tal_topk of 10")
            from ..nn.autograd_ops import DetectionLossFn

            total, items = DetectionLossFn.apply(gt, strides, self.nc, self.reg_max, (self.box, self.cls, self.dfl), *feats)
            return total, items
        out, _ = H.detection_loss(feats, gt, strides, self.nc, self.reg_max, topk=self.topk, box=self.box, cls=self.cls, dfl=self.dfl)
        return out[3], out[:3]


class v8OBBLoss(v8DetectionLoss):
    """Oriented-box training loss on the device (reference: ultralytics/utils/loss.py:612-725 ``v8OBBLoss``): rotated TaskAlignedAssigner +
    BCE / ProbIoU / DFL, value and gradient w.r.t. the head maps AND the angle logits, through ``dy_obb_loss``.

    ``preds`` is ``(feats, angle_levels)``: the per-level fp32 head maps and, per level, the fp32 map whose channel 0 is the RAW angle logit
    (the kernel applies ``(sigmoid - 0.25) * pi`` itself; the reference's training head hands the loss the angle).  The label table has six
    columns ``[cls, x, y, w, h, r]``: xywh in pixels, r in radians."""

    width = 6  # columns of the label table (v8DetectionLoss: 5)

    @staticmethod
    def preprocess(targets: torch.Tensor, batch_size: int, scale_tensor: torch.Tensor) -> torch.Tensor:
        """(N, 7) [image, cls, x, y, w, h normalised, r] -> (B, n_max, 6) [cls, x, y, w, h pixels, r] -- loss.py:621-636, vectorised in numpy on
        the host like the parent's (and for its reason)."""
        t = targets.detach().cpu().float().numpy()
        nl = t.shape[0]
        if nl == 0:
            return torch.zeros(batch_size, 0, 6)
        img = t[:, 0].astype(np.int64)
        counts = np.bincount(img, minlength=batch_size)
        order = np.argsort(img, kind="stable")
        start = np.cumsum(counts) - counts
        pos = np.arange(nl) - start[img[order]]
        out = np.zeros((batch_size, int(counts.max()), 6), dtype=np.float32)
        out[img[order], pos] = t[order, 1:]
        out[..., 1:5] *= scale_tensor.detach().cpu().float().numpy()
        return torch.from_numpy(out)

    def targets_to_gt(self, batch, batch_size: int, img_hw) -> torch.Tensor:
        """The batch's labels as the (B, n_max, 6) table on the host; img_hw = (h, w).  Two rules of the reference's ``__call__`` live here:
        the tiny-box filter (loss.py:660-661) multiplies the normalised WIDTH by the image HEIGHT and the height by the width (``imgsz`` is
        (h, w)) -- kept as it is; and ``mask_gt`` (loss.py:664) is the sign of x + y + w + h + r, so a real label whose five numbers sum to
        zero or less is treated like padding: such rows are dropped here and never reach the table."""
        bboxes = batch["bboxes"].float().cpu()
        if bboxes.dim() != 2 or bboxes.shape[1] != 5:
            raise TypeError(f"the oriented-box loss needs labels whose 'bboxes' are (M, 5) xywhr, got {tuple(bboxes.shape)}")
        t = torch.cat((batch["batch_idx"].view(-1, 1).float().cpu(), batch["cls"].view(-1, 1).float().cpu(), bboxes), 1).numpy()
        h, w = np.float32(img_hw[0]), np.float32(img_hw[1])
        t = t[(t[:, 4] * h >= 2) & (t[:, 5] * w >= 2)]
        scaled = t[:, 2:6] * np.array([w, h, w, h], np.float32)
        t = t[(scaled.sum(1, dtype=np.float32) + t[:, 6]) > 0] if t.shape[0] else t
        gt = self.preprocess(torch.from_numpy(t), batch_size, torch.tensor([float(w), float(h), float(w), float(h)]))
        self.check_classes(gt, self.nc)
        return gt

    def __call__(self, preds, batch):
        feats = preds[0]
        hw = (feats[0].shape[2] * float(self.stride[0]), feats[0].shape[3] * float(self.stride[0]))
        return self.from_gt(preds, self.targets_to_gt(batch, feats[0].shape[0], hw))

    def from_gt(self, preds, gt: torch.Tensor):
        """loss, loss_items from the six-column table itself (host or device, rows with x + y + w + h + r <= 0 = padding)."""
        feats, angles = preds
        self.check_classes(gt, self.nc)
        strides = [float(s) for s in self.stride]
        if any(t.requires_grad for t in (*feats, *angles)):
            if self.topk != 10:
                raise NotImplementedError("the differentiable path uses the default tal_topk of 10")
            from ..nn.autograd_ops import OBBLossFn

            return OBBLossFn.apply(gt, strides, self.nc, self.reg_max, (self.box, self.cls, self.dfl), len(feats), *feats, *angles)
        out, _ = H.obb_loss(feats, angles, gt, strides, self.nc, self.reg_max, topk=self.topk, box=self.box, cls=self.cls, dfl=self.dfl)
        return out[3], out[:3]


class v8SegmentationLoss(v8DetectionLoss):
    """Segmentation training loss on the device (reference: ultralytics/utils/loss.py:263-443 ``v8SegmentationLoss``, ``overlap_mask=True``):
    the detection loss through ``dy_detection_loss`` as the parent runs it, then the mask term through ``dy_seg_loss`` behind its owner map.

    ``preds`` is ``(feats, coef_levels, proto)``: the per-level fp32 head maps, per level the fp32 map of the 32 mask coefficients, and the
    prototypes (N, 32, mh, mw) in the storage type.  ``batch["masks"]``: uint8 / int32 (N, gh, gw) overlap index maps, value k + 1 = the
    image's k-th label in the batch's order (= row k of the label table), with (mh, mw) = (gh, gw) or exactly twice it.  Items come back in
    the reference's order: box, seg, cls, dfl.  The foreground set of the mask term is the owner map's (anchors with a positive alignment
    metric); the reference's zero-metric picks, which follow ``torch.topk``'s tie order, are left out (DESIGN)."""

    width = 5  # the parent's table: [cls, x1, y1, x2, y2]

    def __call__(self, preds, batch):
        feats = preds[0]
        if "masks" not in batch:
            raise TypeError("the segmentation loss needs batch['masks'] (overlap index maps); is this a detection dataset?")
        hw = (feats[0].shape[2] * float(self.stride[0]), feats[0].shape[3] * float(self.stride[0]))
        return self.from_gt(preds, self.targets_to_gt(batch, feats[0].shape[0], hw), batch["masks"])

    def from_gt(self, preds, gt: torch.Tensor, masks: torch.Tensor):
        """loss, loss_items from the label table and the index maps themselves (host or device): the graphed step keeps both in static
        device buffers."""
        feats, coefs, proto = preds
        self.check_classes(gt, self.nc)
        strides = [float(s) for s in self.stride]
        hyp = (self.box, self.cls, self.dfl)
        if any(t.requires_grad for t in (*feats, *coefs, proto)):
            if self.topk != 10:
                raise NotImplementedError("the differentiable path uses the default tal_topk of 10")
            from ..nn.autograd_ops import SegLossFn

            return SegLossFn.apply(gt, masks, strides, self.nc, self.reg_max, hyp, len(feats), *feats, *coefs, proto)
        out, owner = H.detection_loss(feats, gt, strides, self.nc, self.reg_max, topk=self.topk, box=self.box, cls=self.cls, dfl=self.dfl, want_owner=True)
        hw = (feats[0].shape[2] * strides[0], feats[0].shape[3] * strides[0])
        sout = H.seg_loss(owner, gt, coefs, proto, masks, hw, box=self.box, topk=self.topk)
        return out[3] + sout[1], torch.stack((out[0], sout[0], out[1], out[2]))
