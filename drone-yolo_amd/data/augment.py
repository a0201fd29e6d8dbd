"""LetterBox of the predictor's input side (reference: ultralytics/data/augment.py:1486-1620), device version.

Same constructor arguments and the same host geometry as the reference (augment.py:1566-1591); the pixels are produced by
``dy_letterbox_u8_to_nchw_f32``, which also does what BasePredictor.preprocess does next for non-tensor sources
(BGR->RGB, HWC->CHW, float, /255 — engine/predictor.py:125-135), so the output is the model's fp32 NCHW input.
Label updating (``_update_labels``) belongs to the training data pipeline and is not part of the accelerated path.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .. import hip_ops as H


class LetterBox:
    def __init__(self, new_shape=(640, 640), auto=False, scale_fill=False, scaleup=True, center=True, stride=32):
        self.new_shape = (new_shape, new_shape) if isinstance(new_shape, int) else tuple(new_shape)
        self.auto, self.scale_fill, self.scaleup, self.center, self.stride = auto, scale_fill, scaleup, center, int(stride)

    def geometry(self, shape: Tuple[int, int]):
        """(new_w, new_h, top, bottom, left, right) for a (h, w) frame — augment.py:1566-1591."""
        new_shape = self.new_shape
        r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
        if not self.scaleup:
            r = min(r, 1.0)
        new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
        dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
        if self.auto:
            dw, dh = dw % self.stride, dh % self.stride
        elif self.scale_fill:
            dw, dh = 0.0, 0.0
            new_unpad = (new_shape[1], new_shape[0])
        if self.center:
            dw /= 2
            dh /= 2
        top, bottom = (int(round(dh - 0.1)) if self.center else 0), int(round(dh + 0.1))
        left, right = (int(round(dw - 0.1)) if self.center else 0), int(round(dw + 0.1))
        return new_unpad[0], new_unpad[1], top, bottom, left, right

    def into(self, frame: torch.Tensor, out: torch.Tensor, swap_rb: bool = True) -> None:
        """ONE device uint8 (H, W, 3) frame -> ``out``, a (1, 3, Hn, Wn) fp32 slice of a batch tensor whose size is this LetterBox's output
        for the frame: the per-image form ``pre_transform`` uses for sources of different shapes (engine/predictor.py:147-163, auto = False:
        every image letterboxed to the full ``new_shape``)."""
        h0, w0, _ = frame.shape
        nw, nh, top, bottom, left, right = self.geometry((h0, w0))
        if tuple(out.shape) != (1, 3, nh + top + bottom, nw + left + right) or not out.is_contiguous():
            raise ValueError(f"LetterBox.into: out must be a contiguous (1, 3, {nh + top + bottom}, {nw + left + right}) slice")
        H.letterbox(frame[None], nw, nh, top, left, nh + top + bottom, nw + left + right, swap_rb, out=out)

    def __call__(self, frames: torch.Tensor, swap_rb: bool = True) -> torch.Tensor:
        """frames: device uint8 (N, H, W, 3) -> fp32 (N, 3, Hn, Wn) in [0, 1], letterboxed."""
        H.require_device(frames, "frames")
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
            raise ValueError("LetterBox expects a contiguous uint8 (N, H, W, 3) device tensor")
        n, h0, w0, _ = frames.shape
        nw, nh, top, bottom, left, right = self.geometry((h0, w0))
        return H.letterbox(frames, nw, nh, top, left, nh + top + bottom, nw + left + right, swap_rb)


# ---- training augmentation: parameter side and label side (the pixels are dy_augment_u8_nchw's) -----------------------------------------
# Reference: Mosaic (augment.py:490-864), RandomPerspective (:952-1300), RandomHSV (:1303-1390), RandomFlip (:1392-1483), composed by
# v8_transforms (:2287-2351) and closed by Format(normalize=True, bbox_format="xywh").  numpy only: nothing here is a torch CPU op, because
# the per-step host path shares 16 CPUs with the launch of the graphed step.
# one row of dy_augment_u8_nchw's table (dy_aug_row); src[i] = (index, x1a, y1a, x2a, y2a, x1b, y1b, reserved)
AUG_ROW_DTYPE = np.dtype([("n_src", "<i4"), ("ch", "<i4"), ("cw", "<i4"), ("flags", "<i4"), ("src", "<i4", (4, 8)), ("minv", "<f4", (9,)), ("hsv", "<f4", (3,))])
# Rows of one image's label table the training step accepts.  Nothing in dy_detection_loss bounds gmax structurally (its workspace and grids
# are sized from it), but the assigner's cost grows with gmax^2 and every set trained so far had <= 300 rows per image; a mosaic carries four
# images' boxes: 4 x 300 rounded up to the label table's granularity of 64 rows.
MAX_LABEL_ROWS = 1216
AUG_KEYS = ("mosaic", "close_mosaic", "degrees", "translate", "scale", "shear", "perspective", "hsv_h", "hsv_s", "hsv_v", "fliplr", "flipud")


def mosaic_placement(s: int, yc: int, xc: int, shapes):
    """Mosaic._mosaic4 (augment.py:684-708) for four (h, w) images around the centre (yc, xc) of a 2s x 2s canvas: per image the canvas
    rectangle a = (x1a, y1a, x2a, y2a), the source rectangle b = (x1b, y1b, x2b, y2b) and the label shift (padw, padh) = (x1a - x1b, y1a - y1b)."""
    a, b, pads = [], [], []
    for i, (h, w) in enumerate(shapes):
        if i == 0:  # top left: the image's bottom-right corner on the centre
            ra = (max(xc - w, 0), max(yc - h, 0), xc, yc)
            rb = (w - (ra[2] - ra[0]), h - (ra[3] - ra[1]), w, h)
        elif i == 1:  # top right
            ra = (xc, max(yc - h, 0), min(xc + w, s * 2), yc)
            rb = (0, h - (ra[3] - ra[1]), min(w, ra[2] - ra[0]), h)
        elif i == 2:  # bottom left
            ra = (max(xc - w, 0), yc, xc, min(s * 2, yc + h))
            rb = (w - (ra[2] - ra[0]), 0, w, min(ra[3] - ra[1], h))
        else:  # bottom right
            ra = (xc, yc, min(xc + w, s * 2), min(s * 2, yc + h))
            rb = (0, 0, min(w, ra[2] - ra[0]), min(ra[3] - ra[1], h))
        a.append(ra), b.append(rb), pads.append((ra[0] - rb[0], ra[1] - rb[1]))
    return a, b, pads


def center_placement(s: int, shape):
    """The non-mosaic branch: one (h, w) image centred on the s x s canvas, the padding of LetterBox(new_shape=(s, s), center=True) at ratio 1
    (augment.py:1585-1591).  Same (a, b, pad) triple as one entry of ``mosaic_placement``; an image larger than the canvas is cropped."""
    h, w = shape
    left, top = int(round((s - w) / 2 - 0.1)), int(round((s - h) / 2 - 0.1))
    x1a, y1a, x2a, y2a = max(left, 0), max(top, 0), min(left + w, s), min(top + h, s)
    return (x1a, y1a, x2a, y2a), (x1a - left, y1a - top, x2a - left, y2a - top), (left, top)


def rotation_matrix_2d(angle: float, scale: float) -> np.ndarray:
    """cv2.getRotationMatrix2D(angle=a, center=(0, 0), scale=s) (2 x 3, float64; a in degrees, positive = counter-clockwise with the y axis down)."""
    al, be = scale * math.cos(math.radians(angle)), scale * math.sin(math.radians(angle))
    return np.array([[al, be, 0.0], [-be, al, 0.0]], dtype=np.float64)


def affine_matrix(canvas_hw, size_wh, angle=0.0, scale=1.0, shear_x=0.0, shear_y=0.0, persp_x=0.0, persp_y=0.0, tx=0.5, ty=0.5) -> np.ndarray:
    """M = T S R P C of RandomPerspective.affine_transform (augment.py:1041-1071), float32 factors multiplied in float32 as there.
    ``canvas_hw``: the image being warped; ``size_wh``: the output; shears in degrees; (tx, ty): the drawn fractions of the output size."""
    c = np.eye(3, dtype=np.float32)
    c[0, 2], c[1, 2] = -canvas_hw[1] / 2, -canvas_hw[0] / 2
    p = np.eye(3, dtype=np.float32)
    p[2, 0], p[2, 1] = persp_x, persp_y
    r = np.eye(3, dtype=np.float32)
    r[:2] = rotation_matrix_2d(angle, scale)
    sh = np.eye(3, dtype=np.float32)
    sh[0, 1], sh[1, 0] = math.tan(shear_x * math.pi / 180), math.tan(shear_y * math.pi / 180)
    t = np.eye(3, dtype=np.float32)
    t[0, 2], t[1, 2] = tx * size_wh[0], ty * size_wh[1]
    return t @ sh @ r @ p @ c


def inverse_matrix(m: np.ndarray) -> np.ndarray:
    """The kernel's output -> canvas map: M inverted in float64, stored as float32 (row-major 9 values)."""
    return np.linalg.inv(m.astype(np.float64)).astype(np.float32).reshape(9)


def _xywh2xyxy(x: np.ndarray) -> np.ndarray:
    y = np.empty_like(x)
    half = x[..., 2:] / 2
    y[..., :2] = x[..., :2] - half
    y[..., 2:] = x[..., :2] + half
    return y


def _xyxy2xywh(x: np.ndarray) -> np.ndarray:
    y = np.empty_like(x)
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def _clip_xyxy(b: np.ndarray, w, h) -> None:
    b[:, [0, 2]] = b[:, [0, 2]].clip(0, w)
    b[:, [1, 3]] = b[:, [1, 3]].clip(0, h)


def place_labels(sources, canvas_hw, cat: bool = True):
    """``sources``: per pasted image (cls (n,) or (n, 1), normalised xywh boxes (n, 4) float32, (h, w), (padw, padh)).  Per source
    Mosaic._update_labels (augment.py:809-812: xyxy, times (w, h), plus the shift); ``cat`` (the mosaic branch): concatenated, clipped to the
    canvas, zero-area boxes dropped (_cat_labels, augment.py:859-861).  Returns (cls (n, 1), xyxy (n, 4) float32 in canvas pixels)."""
    cls, boxes = [], []
    for c, bb, (h, w), (padw, padh) in sources:
        b = _xywh2xyxy(np.asarray(bb, dtype=np.float32).reshape(-1, 4))
        b[:, 0] *= w
        b[:, 1] *= h
        b[:, 2] *= w
        b[:, 3] *= h
        b[:, 0] += padw
        b[:, 1] += padh
        b[:, 2] += padw
        b[:, 3] += padh
        cls.append(np.asarray(c, dtype=np.float32).reshape(-1, 1)), boxes.append(b)
    cls, boxes = np.concatenate(cls, 0), np.concatenate(boxes, 0)
    if cat:
        _clip_xyxy(boxes, canvas_hw[1], canvas_hw[0])
        good = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) > 0
        cls, boxes = cls[good], boxes[good]
    return cls, boxes


def apply_matrix_to_boxes(boxes: np.ndarray, m: np.ndarray, perspective: bool) -> np.ndarray:
    """RandomPerspective.apply_bboxes (augment.py:1100-1112): the four corners through M (divided by the third coordinate only when the
    ``perspective`` argument is non-zero), the new box their axis-aligned hull."""
    n = len(boxes)
    if n == 0:
        return boxes
    xy = np.ones((n * 4, 3), dtype=boxes.dtype)
    xy[:, :2] = boxes[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2)
    xy = xy @ m.T
    xy = (xy[:, :2] / xy[:, 2:3] if perspective else xy[:, :2]).reshape(n, 8)
    x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
    return np.concatenate((x.min(1), y.min(1), x.max(1), y.max(1)), dtype=boxes.dtype).reshape(4, n).T


def box_candidates(box1: np.ndarray, box2: np.ndarray, wh_thr=2, ar_thr=100, area_thr=0.1, eps=1e-16) -> np.ndarray:
    """augment.py:1297-1300; box1 before (scaled), box2 after, both (4, n)."""
    w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
    w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    return (w2 > wh_thr) & (h2 > wh_thr) & (w2 * h2 / (w1 * h1 + eps) > area_thr) & (ar < ar_thr)


def warp_labels(boxes: np.ndarray, m: np.ndarray, scale: float, size_wh, perspective: bool):
    """RandomPerspective.__call__'s label path (augment.py:1237-1258): boxes through M, clipped to the output, kept where
    box_candidates(before * scale, after, area_thr = 0.10) holds.  Returns (new boxes (n, 4), kept mask (n,))."""
    new = apply_matrix_to_boxes(boxes, m, perspective)
    if len(new) == 0:
        return new, np.zeros((0,), dtype=bool)
    new = np.array(new)
    _clip_xyxy(new, size_wh[0], size_wh[1])
    before = boxes.copy()
    before[:, 0] *= scale
    before[:, 1] *= scale
    before[:, 2] *= scale
    before[:, 3] *= scale
    return new, box_candidates(before.T, new.T, area_thr=0.10)


def flip_and_normalise(boxes: np.ndarray, size_wh, flipud: bool, fliplr: bool) -> np.ndarray:
    """RandomFlip.__call__ (vertical first, then horizontal, as v8_transforms orders them) on xywh pixel boxes, then Format's normalised xywh."""
    w, h = size_wh
    b = _xyxy2xywh(boxes)
    if flipud:
        b[:, 1] = h - b[:, 1]
    if fliplr:
        b[:, 0] = w - b[:, 0]
    b[:, 0] *= 1 / w
    b[:, 1] *= 1 / h
    b[:, 2] *= 1 / w
    b[:, 3] *= 1 / h
    return b


def transform_labels(sources, canvas_hw, m: np.ndarray, scale: float, size_wh, perspective: bool = False, flipud: bool = False, fliplr: bool = False):
    """The reference's label path for ONE output image, in its order: place (and, for a mosaic = several sources, concatenate / clip / drop
    zero-area), warp with M and filter, flip, normalise.  Returns (cls (k, 1) float32, normalised xywh (k, 4) float32)."""
    cls, boxes = place_labels(sources, canvas_hw, cat=len(sources) > 1)
    new, keep = warp_labels(boxes, m, scale, size_wh, perspective)
    return cls[keep], flip_and_normalise(new[keep], size_wh, flipud, fliplr)


class DeviceAugment:
    """Owns the random draws and builds, per batch, the kernel's table and the labels.  Every output sample draws from its own
    ``numpy.random.Generator`` seeded with (seed, epoch, dataset index): a sample does not depend on the batch size, the number of ranks or
    on where a resumed run starts.  Ranges as the reference: mosaic centre int(uniform(S/2, 3S/2)) per axis (border = -S/2, augment.py:684),
    three partners uniform over the dataset, angle uniform(-degrees, degrees), scale uniform(1 - scale, 1 + scale), shears, perspective
    terms, translation uniform(0.5 - translate, 0.5 + translate) x S, HSV offsets uniform(-1, 1) x (hsv_h, hsv_s, hsv_v) x (180, 255, 255),
    flips by probability, ``mosaic`` the probability of the four-image branch.  The reference's global random stream is not reproduced."""

    def __init__(self, args: dict, imgsz: int, data: dict, seed: int = 0):
        self.s = int(imgsz)
        if self.s % 4:
            raise ValueError(f"device_augment: imgsz = {self.s} must be a multiple of 4")
        self.hyp = {k: args[k] for k in AUG_KEYS}
        self.seed = int(seed)
        img = data["img"]
        self.n, _, self.hs, self.ws = (int(v) for v in img.shape)
        bi = np.asarray(data["batch_idx"], dtype=np.int64).reshape(-1)
        order = np.argsort(bi, kind="stable")
        self.cls = np.asarray(data["cls"], dtype=np.float32).reshape(-1)[order]
        self.boxes = np.asarray(data["bboxes"], dtype=np.float32).reshape(-1, 4)[order]
        counts = np.bincount(bi, minlength=self.n)
        self.start = np.concatenate(([0], np.cumsum(counts)))
        self.max_count = int(counts.max()) if self.n else 0
        rect = data.get("rect")
        self.rect = np.asarray(rect, dtype=np.int64).reshape(-1, 4) if rect is not None else np.tile(np.array([0, 0, self.hs, self.ws]), (self.n, 1))
        if len(self.rect) != self.n:
            raise ValueError("dataset 'rect' must be (N, 4) int32 (top, left, h, w)")

    def label_bound(self) -> int:
        """Rows one output image can carry at most: four images' labels (partners are drawn with replacement)."""
        return 4 * self.max_count if self.hyp["mosaic"] > 0 else self.max_count

    def _labels_of(self, i: int):
        """(cls, normalised xywh relative to the image's valid region, (h, w) of the region)."""
        c, b = self.cls[self.start[i] : self.start[i + 1]], self.boxes[self.start[i] : self.start[i + 1]]
        top, left, h, w = (int(v) for v in self.rect[i])
        if (top, left, h, w) != (0, 0, self.hs, self.ws):  # stored normalised to the whole square: re-express on the region
            b = b.copy()
            b[:, 0] = (b[:, 0] * self.ws - left) / w
            b[:, 1] = (b[:, 1] * self.hs - top) / h
            b[:, 2] = b[:, 2] * self.ws / w
            b[:, 3] = b[:, 3] * self.hs / h
        return c, b, (h, w)

    def draw(self, epoch: int, index: int, mosaic_on: bool = True) -> dict:
        """The parameters of output sample (epoch, index)."""
        hy, s = self.hyp, self.s
        g = np.random.default_rng([self.seed, int(epoch), int(index)])
        d = dict(index=int(index))
        d["mosaic"] = bool(g.random() < hy["mosaic"]) and mosaic_on
        d["partners"] = [int(v) for v in g.integers(0, self.n, 3)]
        d["yc"], d["xc"] = (int(g.uniform(s / 2, 3 * s / 2)) for _ in range(2))
        d["persp"] = (g.uniform(-hy["perspective"], hy["perspective"]), g.uniform(-hy["perspective"], hy["perspective"]))
        d["angle"] = g.uniform(-hy["degrees"], hy["degrees"])
        d["scale"] = g.uniform(1 - hy["scale"], 1 + hy["scale"])
        d["shear"] = (g.uniform(-hy["shear"], hy["shear"]), g.uniform(-hy["shear"], hy["shear"]))
        d["t"] = (g.uniform(0.5 - hy["translate"], 0.5 + hy["translate"]), g.uniform(0.5 - hy["translate"], 0.5 + hy["translate"]))
        d["hsv"] = g.uniform(-1, 1, 3) * (hy["hsv_h"], hy["hsv_s"], hy["hsv_v"]) * (180, 255, 255)
        d["flipud"], d["fliplr"] = bool(g.random() < hy["flipud"]), bool(g.random() < hy["fliplr"])
        return d

    def sample(self, epoch: int, index: int, row: np.void, mosaic_on: bool = True, remap=None):
        """Fill table row ``row`` for output sample (epoch, index) and return its labels (cls (k, 1), normalised xywh (k, 4)).
        ``remap``: dataset index -> position in the uploaded source tensor (the per-batch-upload mode); None = the dataset is resident."""
        d, s = self.draw(epoch, index, mosaic_on), self.s
        ids = [d["index"]] + d["partners"] if d["mosaic"] else [d["index"]]
        labs = [self._labels_of(i) for i in ids]
        shapes = [hw for _, _, hw in labs]
        if d["mosaic"]:
            canvas = (2 * s, 2 * s)
            a, b, pads = mosaic_placement(s, d["yc"], d["xc"], shapes)
        else:
            canvas = (s, s)
            a1, b1, p1 = center_placement(s, shapes[0])
            a, b, pads = [a1], [b1], [p1]
        m = affine_matrix(canvas, (s, s), d["angle"], d["scale"], d["shear"][0], d["shear"][1], d["persp"][0], d["persp"][1], d["t"][0], d["t"][1])
        hsv_on = bool(self.hyp["hsv_h"] or self.hyp["hsv_s"] or self.hyp["hsv_v"])
        row["n_src"], row["ch"], row["cw"] = len(ids), canvas[0], canvas[1]
        row["flags"] = (_lib.DY_AUG_FLIPLR if d["fliplr"] else 0) | (_lib.DY_AUG_FLIPUD if d["flipud"] else 0) | (0 if hsv_on else _lib.DY_AUG_HSV_OFF)
        row["src"] = 0
        for k, i in enumerate(ids):
            top, left = int(self.rect[i][0]), int(self.rect[i][1])
            row["src"][k] = (i if remap is None else remap[i], a[k][0], a[k][1], a[k][2], a[k][3], b[k][0] + left, b[k][1] + top, 0)
        row["minv"] = inverse_matrix(m)
        row["hsv"] = d["hsv"]
        cls, boxes = transform_labels([(c, bb, hw, pads[k]) for k, (c, bb, hw) in enumerate(labs)], canvas, m, d["scale"], (s, s),
                                      perspective=bool(self.hyp["perspective"]), flipud=d["flipud"], fliplr=d["fliplr"])
        if len(cls) > MAX_LABEL_ROWS:
            raise ValueError(f"device_augment: sample {index} of epoch {epoch} carries {len(cls)} label rows, more than the {MAX_LABEL_ROWS} "
                             "rows per image the training step takes (data.augment.MAX_LABEL_ROWS)")
        return cls, boxes

    def sources_of(self, epoch: int, indices, mosaic_on: bool = True):
        """The dataset images a batch reads, sorted and unique (the per-batch-upload mode uploads exactly these)."""
        need = set()
        for i in indices:
            d = self.draw(epoch, i, mosaic_on)
            need.update([d["index"]] + (d["partners"] if d["mosaic"] else []))
        return sorted(need)

    def build(self, epoch: int, indices, mosaic_on: bool = True, remap=None):
        """Table (len(indices),) of AUG_ROW_DTYPE and the batch's labels in the collate layout (numpy: batch_idx (M,), cls (M, 1), bboxes (M, 4))."""
        table = np.zeros(len(indices), dtype=AUG_ROW_DTYPE)
        bi, cls, boxes = [], [], []
        for j, i in enumerate(indices):
            c, b = self.sample(epoch, i, table[j], mosaic_on, remap)
            bi.append(np.full((len(c),), float(j), dtype=np.float32)), cls.append(c), boxes.append(b)
        return table, dict(batch_idx=np.concatenate(bi) if bi else np.zeros((0,), np.float32),
                           cls=np.concatenate(cls, 0) if cls else np.zeros((0, 1), np.float32),
                           bboxes=np.concatenate(boxes, 0) if boxes else np.zeros((0, 4), np.float32))


def launch_augment(src: torch.Tensor, table: np.ndarray, s: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Upload ``table`` and run dy_augment_u8_nchw over device sources ``src`` (N, 3, Hs, Ws) uint8 -> (len(table), 3, s, s) uint8."""
    assert table.dtype == AUG_ROW_DTYPE and table.flags["C_CONTIGUOUS"]
    dev = torch.from_numpy(table.view(np.uint8).reshape(len(table), AUG_ROW_DTYPE.itemsize)).to(src.device, non_blocking=True)
    return H.augment_batch(src, dev, s, out=out)
