"""Host arithmetic of ``predict(frames, crops=boxes)``: the expanded integer crop rectangle of a box and the table
``dy_crops_letterbox_u8_to_nchw_f32`` reads.  Nothing here touches a device.

The rectangle is the drone-video pipeline's (mix6.py:94-101): the box grown by ``expand`` times its width / height on every side, cut at the
frame and truncated to integers, in Python floats.  The letterbox geometry of a crop is ``LetterBox(auto=False)`` on an image of the crop's
shape -- what the predictor does for a list of images of different shapes, so every crop becomes one ``imgsz x imgsz`` input.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

CROP_COLS = 9  # frame, x0, y0, cw, ch, new_w, new_h, top, left


def crop_rect(box: Sequence[float], frame_hw: Tuple[int, int], expand: float) -> Tuple[int, int, int, int]:
    """(x0, y0, x1e, y1e) of an xyxy box in a (H, W) frame."""
    x1, y1, x2, y2 = (float(v) for v in box)
    w, h = x2 - x1, y2 - y1
    r = float(expand)
    return (int(max(0, x1 - w * r)), int(max(0, y1 - h * r)), int(min(frame_hw[1], x2 + w * r)), int(min(frame_hw[0], y2 + h * r)))


def as_frames(source) -> list:
    """``source`` as a list of HWC uint8 frames of ONE shape; ``ValueError`` for anything else (a tensor among them)."""
    if type(source).__module__.startswith("torch"):
        raise ValueError("crops: the frames must be uint8 HWC numpy arrays ((F, H, W, 3) or a list of one shape), not a tensor")
    if isinstance(source, np.ndarray):
        frames = [source] if source.ndim == 3 else list(source)
    elif isinstance(source, (list, tuple)) and len(source) > 0 and all(isinstance(f, np.ndarray) for f in source):
        frames = list(source)
    else:
        raise ValueError("crops: the frames must be uint8 HWC numpy arrays ((F, H, W, 3) or a list of one shape)")
    for f in frames:
        if f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
            raise ValueError("crops: the frames must be uint8 HWC BGR frames")
    if len({f.shape for f in frames}) != 1:
        raise ValueError(f"crops: the frames must have one shape, got {sorted({f.shape for f in frames})}")
    return frames


def crop_rects(frames: list, boxes, expand: float) -> List[Tuple[int, int, int, int, int]]:
    """(frame, x0, y0, x1e, y1e) of every box, frame by frame in box order; ``ValueError`` for an empty crop or boxes that do not fit the frames."""
    if not isinstance(boxes, (list, tuple)) or len(boxes) != len(frames):
        raise ValueError(f"crops: one (n_i, 4) array of xyxy boxes per frame is expected ({len(frames)} frames)")
    hw = frames[0].shape[:2]
    rects = []
    for f, bx in enumerate(boxes):
        if type(bx).__module__.startswith("torch") and bx.is_cuda:
            raise ValueError("crops: the boxes must be host arrays")
        bx = np.asarray(bx, dtype=np.float64).reshape(-1, 4) if np.size(bx) else np.zeros((0, 4))
        for j, b in enumerate(bx):
            x0, y0, x1, y1 = crop_rect(b, hw, expand)
            if x1 <= x0 or y1 <= y0:
                raise ValueError(f"crops: box {j} of frame {f} ({[float(v) for v in b]}) gives an empty crop of the {hw[1]}x{hw[0]} frame")
            rects.append((f, x0, y0, x1, y1))
    if not rects:
        raise ValueError("crops: no boxes")
    return rects


def crop_table(rects, imgsz: int, stride: int = 32) -> np.ndarray:
    """int32 (k, 9) rows  frame, x0, y0, cw, ch, new_w, new_h, top, left  of ``rects`` for ``imgsz x imgsz`` inputs."""
    from ..data.augment import LetterBox

    lb = LetterBox(imgsz, auto=False, stride=stride)
    table = np.zeros((len(rects), CROP_COLS), dtype=np.int32)
    for i, (f, x0, y0, x1, y1) in enumerate(rects):
        cw, ch = x1 - x0, y1 - y0
        nw, nh, top, _, left, _ = lb.geometry((ch, cw))
        table[i] = (f, x0, y0, cw, ch, nw, nh, top, left)
    return table
