"""The float64 reference of the mask assembly (``dy_process_mask``), shared by tools/make_seg_golden.py (which records it next to the real
reference's masks in tests/golden/seg.npz) and by the geometry sweep (tests/test_mask_geometry_host.py / _gpu.py), which evaluates it at
run time.  Plain numpy and CPU torch; not collected.

The semantics are the reference's ``ops.process_mask(upsample=True)`` (crop at proto resolution with the box times mw / iw, zeros blended
in, bilinear resize, > 0), ``ops.process_mask_native`` / ``ops.scale_masks`` (window of the grid resized, > 0, crop at the output) and
``ops.crop_mask`` (``x1 <= x < x2``, ``y1 <= y < y2``; every comparison with a NaN is false, so a box with a NaN corner has an empty mask).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

UNSURE = 64.0 * 2.0 ** -23
NM = 32


# ---- float64 evaluation of the mask blend (value v and magnitude S per output pixel) -------------------------------------------
def blend64(protos, coef, boxes, window, out_hw, crop_ratio=None, *, half_pixel=True, clamp_x1=True):
    """protos (mh, mw, 32), coef (n, 32), boxes (n, 4) -> v, S (n, oh, ow) in float64.  ``crop_ratio`` = (rx, ry): corners outside the box
    times the ratio count as zero (ops.process_mask); None: no corner crop (ops.process_mask_native).

    ``half_pixel`` / ``clamp_x1`` are the checker's mutation knobs (tests/test_mask_geometry_host.py), both True in every reference:
    False leaves the half-pixel offset out (``src = scale * dst``) / lets the right corner column run past the window, where it reads what
    lies there in memory (the grid's next pixel in row-major order, zeros behind the grid)."""
    p = np.asarray(protos, np.float64)
    c = np.asarray(coef, np.float64)
    top, left, sh, sw = window
    if not clamp_x1:  # column sw of the window: pixel (top + y, left + sw) of the row-major grid
        mh, mw = p.shape[:2]
        flat = np.concatenate([p.reshape(mh * mw, -1), np.zeros((mw + 1, p.shape[2]))], 0)
        extra = flat[(top + np.arange(sh)) * mw + left + sw]
    p = p[top : top + sh, left : left + sw]
    if not clamp_x1:
        p = np.concatenate([p, extra[:, None, :]], 1)
    oh, ow = out_hw
    val = np.einsum("nk,yxk->nyx", c, p)
    mag = np.einsum("nk,yxk->nyx", np.abs(c), np.abs(p))
    if crop_ratio is not None:
        b = np.asarray(boxes, np.float32).astype(np.float64)
        x1, x2 = b[:, 0] * crop_ratio[0] - left, b[:, 2] * crop_ratio[0] - left
        y1, y2 = b[:, 1] * crop_ratio[1] - top, b[:, 3] * crop_ratio[1] - top
        xs, ys = np.arange(p.shape[1])[None, None, :], np.arange(sh)[None, :, None]
        keep = (xs >= x1[:, None, None]) & (xs < x2[:, None, None]) & (ys >= y1[:, None, None]) & (ys < y2[:, None, None])
        val, mag = val * keep, mag * keep

    def axis(s, o, clamp=True):
        src = (np.arange(o) + (0.5 if half_pixel else 0.0)) * (np.float32(s) / np.float32(o)).astype(np.float64) - (0.5 if half_pixel else 0.0)
        src = np.maximum(src, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), s - 1)
        i1 = np.minimum(i0 + 1, s - 1) if clamp else i0 + 1
        l1 = src - i0
        return i0, i1, 1.0 - l1, l1

    y0, y1_, ly0, ly1 = axis(sh, oh)
    x0, x1_, lx0, lx1 = axis(sw, ow, clamp_x1)

    def mix(a):
        t = a[:, y0][:, :, x0] * lx0 + a[:, y0][:, :, x1_] * lx1
        b_ = a[:, y1_][:, :, x0] * lx0 + a[:, y1_][:, :, x1_] * lx1
        return t * ly0[None, :, None] + b_ * ly1[None, :, None]

    return mix(val), mix(mag)


def in_box(boxes, out_hw):
    """(n, oh, ow) bool: output pixels with x1 <= x < x2 and y1 <= y < y2 (crop_mask on the output grid)."""
    b = np.asarray(boxes, np.float64)
    xs, ys = np.arange(out_hw[1])[None, None, :], np.arange(out_hw[0])[None, :, None]
    return (xs >= b[:, 0, None, None]) & (xs < b[:, 2, None, None]) & (ys >= b[:, 1, None, None]) & (ys < b[:, 3, None, None])


def edges_clear(boxes, ratio, lo=1e-2, clip_hw=None):
    """No crop edge within ``lo`` of an integer.  ``clip_hw``: edges that clip_boxes put exactly on the image border do not count (every
    pixel of the grid is on the same side of them whatever the rounding)."""
    e = np.asarray(boxes, np.float64) * np.array([ratio[0], ratio[1], ratio[0], ratio[1]])
    near = np.abs(e - np.round(e)) <= lo
    if clip_hw is not None:
        lim = np.array([clip_hw[1], clip_hw[0], clip_hw[1], clip_hw[0]], np.float64)
        near &= ~((e == 0) | (e == lim))
    return not bool(near.any())


# ---- the whole batch, composed as tools/make_seg_golden.py::pm_case composes it ---------------------------------------------------
def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def reference_masks(protos, coef, boxes, counts, windows, out_hw, mode, ratio=None, **knobs):
    """protos (n, mh, mw, 32), coef (n, max_det, 32), boxes (n, max_det, 4), ``counts[b]`` rows of image b, ``windows[b]`` = (top, left, sh,
    sw) -> (ref, unsure, inbox), bool (T, oh, ow), T = sum(counts), image after image.

    ``mode`` 'default': boxes in input-image pixels, ``ratio`` = (mw / iw, mh / ih), corners outside the box times the ratio are zero,
    ref = v > 0.  'retina' / 'window': boxes in output pixels, no corner crop, ref = (v > 0) & in_box.  unsure = |v| < UNSURE * S with v, S
    times in_box in the retina and window forms (outside the box the mask is zero whatever v is).  ``inbox`` is the box on the output grid
    (default form: the box times ratio times ow / sw, oh / sh — the box itself where the output is the input image); it only serves as the
    denominator of the unsure share.  Boxes are rounded to float32 first, as the kernel reads them; NaN corners compare false: empty mask.
    ``knobs`` go to ``blend64`` (mutations)."""
    protos, coef = _np(protos), _np(coef)
    boxes = _np(boxes).astype(np.float32)
    oh, ow = out_hw
    ref, unsure, inbox = [], [], []
    with np.errstate(invalid="ignore"):
        for b, k in enumerate(counts):
            win = tuple(int(v) for v in windows[b])
            bx = boxes[b, :k]
            if mode == "default":
                v, s = blend64(protos[b], coef[b, :k], bx, win, out_hw, crop_ratio=ratio, **knobs)
                sx, sy = ratio[0] * ow / win[3], ratio[1] * oh / win[2]
                off = np.array([win[1], win[0], win[1], win[0]], np.float64) * np.array([ow / win[3], oh / win[2]] * 2)
                inb = in_box(bx.astype(np.float64) * np.array([sx, sy, sx, sy]) - off, out_hw)
                r = v > 0
            else:
                v, s = blend64(protos[b], coef[b, :k], bx, win, out_hw, **knobs)
                inb = in_box(bx, out_hw)
                v, s = v * inb, s * inb
                r = (v > 0) & inb
            ref.append(r), unsure.append(np.abs(v) < UNSURE * s), inbox.append(inb)
    return tuple(np.concatenate(a, 0) for a in (ref, unsure, inbox))


def fp32_masks(protos, coef, boxes, counts, windows, out_hw, mode, ratio=None):
    """The same chain in CPU fp32 torch, as the reference runs it (utils/ops.py: process_mask / process_mask_native / scale_masks /
    crop_mask): ``coef @ protos``, crop at proto resolution or window slice, ``F.interpolate(bilinear, align_corners=False)``, ``> 0``,
    ``& in_box`` in the retina and window forms.  Returns bool (T, oh, ow)."""
    protos, coef = torch.as_tensor(_np(protos)).float(), torch.as_tensor(_np(coef)).float()
    boxes = torch.as_tensor(_np(boxes).astype(np.float32))
    n, mh, mw, nm = protos.shape
    out = []
    for b, k in enumerate(counts):
        if not k:
            continue
        top, left, sh, sw = (int(v) for v in windows[b])
        pc = protos[b].permute(2, 0, 1).contiguous()
        m = (coef[b, :k] @ pc.view(nm, -1)).view(-1, mh, mw)
        bx = boxes[b, :k]
        if mode == "default":  # the box in proto pixels, an fp32 product as the kernel's; zeros outside it are blended in
            m = m * _in_box32(bx * torch.tensor([ratio[0], ratio[1], ratio[0], ratio[1]], dtype=torch.float32), (mh, mw))
            m = F.interpolate(m[None, :, top : top + sh, left : left + sw], tuple(out_hw), mode="bilinear", align_corners=False)[0]
            out.append((m > 0).numpy())
        else:
            m = F.interpolate(m[None, :, top : top + sh, left : left + sw], tuple(out_hw), mode="bilinear", align_corners=False)[0]
            out.append(((m > 0) & _in_box32(bx, out_hw)).numpy())
    return np.concatenate(out, 0) if out else np.zeros((0, *out_hw), bool)


def _in_box32(boxes, hw):
    """``in_box`` in fp32 torch: (n, h, w) bool, pixel coordinates compared as fp32 against the fp32 box."""
    xs = torch.arange(hw[1], dtype=torch.float32).view(1, 1, -1)
    ys = torch.arange(hw[0], dtype=torch.float32).view(1, -1, 1)
    lo_x, lo_y, hi_x, hi_y = (boxes[:, i].view(-1, 1, 1) for i in range(4))
    return (xs >= lo_x) & (xs < hi_x) & (ys >= lo_y) & (ys < hi_y)


def make_boxes(rng, k, w, h, ratio):
    """k random float32 boxes, sides 0.3-0.9 of the image, centres 0.1-0.9, redrawn until no crop edge times ``ratio`` lies within 1e-2 of
    an integer."""
    while True:
        cx, cy = rng.uniform(0.1 * w, 0.9 * w, k), rng.uniform(0.1 * h, 0.9 * h, k)
        bw, bh = rng.uniform(0.3 * w, 0.9 * w, k), rng.uniform(0.3 * h, 0.9 * h, k)
        boxes = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1).astype(np.float32)
        if edges_clear(boxes, ratio):
            return boxes


def check_masks(got, ref, unsure, inbox):
    """``wrong``: pixels of the whole masks that differ from the reference outside the unsure set (the bar: 0)."""
    got, ref = np.asarray(got).astype(bool), np.asarray(ref).astype(bool)
    differ = got != ref
    return {"wrong": int((differ & ~unsure).sum()), "differ_in_unsure": int((differ & unsure).sum()),
            "unsure_share": float((unsure & inbox).sum()) / max(int(inbox.sum()), 1), "set": int(ref.sum())}


# ---- the geometry sweep's cases ---------------------------------------------------------------------------------------------------
def degenerate_boxes(w, h, ratio):
    """Boxes whose mask does not depend on any rounding (exempt from the edge clearance): inverted, wholly left of the image, wholly below
    it, zero width, the whole image with corners at -+1e30, a NaN x1, and one narrower than a proto pixel between two integer columns."""
    col = (int(0.4 * w * ratio[0]) + 0.3) / ratio[0], (int(0.4 * w * ratio[0]) + 0.7) / ratio[0]
    return np.array([
        [0.7 * w + 0.37, 0.2 * h + 0.31, 0.3 * w + 0.41, 0.8 * h + 0.27],
        [-0.5 * w - 0.37, 0.2 * h + 0.31, -3.3, 0.8 * h + 0.27],
        [0.2 * w + 0.37, h + 2.6, 0.8 * w + 0.41, 1.5 * h + 0.27],
        [0.4 * w + 0.37, 0.2 * h + 0.31, 0.4 * w + 0.37, 0.8 * h + 0.27],
        [-1e30, -1e30, 1e30, 1e30],
        [float("nan"), 0.2 * h + 0.31, 0.8 * w + 0.41, 0.8 * h + 0.27],
        [col[0], 0.2 * h + 0.31, col[1], 0.8 * h + 0.27],
    ], np.float32)


def _case(tag, mode, grid, window, in_hw, out_hw, counts, max_det, seed, degenerate=None):
    return dict(tag=tag, mode=mode, grid=grid, window=window, in_hw=in_hw, out_hw=out_hw, counts=counts, max_det=max_det, seed=seed, degenerate=degenerate)


# window None: the whole grid.  degenerate = (image, how many of degenerate_boxes): they fill the image's last rows, behind its random boxes.
# Seeds: the first from 2000 on with which the case meets the conditions of tests/test_mask_geometry_host.py (R3, R6, D1: and with which
# every mutation of test_checker_flags_mutations that can change the case changes it).
PM_CASES = [
    _case("R1", "window", (8, 8), None, None, (2, 3), [3, 2], 4, 2000),
    _case("R2", "window", (8, 8), None, None, (3, 5), [8, 1], 8, 2000),
    _case("R3", "window", (12, 8), None, None, (40, 5), [3], 4, 2000),
    _case("R4", "window", (12, 8), None, None, (31, 9), [2, 2], 4, 2000),
    _case("R5", "window", (40, 52), (3, 2, 33, 47), None, (23, 37), [3, 0, 2], 4, 2000),
    # R5's geometry with room for the degenerate boxes (R5 itself has 3 rows in its first image): 2 random + 6 degenerate
    _case("R5d", "window", (40, 52), (3, 2, 33, 47), None, (23, 37), [8, 0, 2], 8, 2000, degenerate=(0, 6)),
    _case("R6", "window", (160, 160), (0, 1, 160, 158), None, (43, 41), [2, 3], 4, 2011),
    _case("R7a", "window", (16, 16), (5, 7, 1, 1), None, (16, 24), [2], 2, 2000),
    _case("R7b", "window", (16, 32), (4, 0, 1, 32), None, (9, 40), [2], 2, 2000),
    _case("R8", "window", (24, 32), None, None, (150, 227), [2, 1], 4, 2000),
    _case("R9", "window", (160, 160), (20, 0, 120, 160), None, (540, 720), [2, 1], 2, 2000),
    _case("D1", "default", (10, 13), None, (40, 52), (40, 52), [4, 8], 8, 2004, degenerate=(1, 7)),
    _case("D2", "default", (24, 32), None, (96, 128), (75, 113), [3, 3], 4, 2000),
    _case("D3", "default", (20, 26), None, (40, 52), (40, 52), [2, 2], 4, 2000),
    _case("D4", "default", (40, 52), None, (160, 208), (23, 37), [3], 4, 2000),
]
PM_TAGS = [c["tag"] for c in PM_CASES]


def pm_case(tag):
    return next(c for c in PM_CASES if c["tag"] == tag)


def case_inputs(case, seed=None):
    """A case's inputs, regenerated from its seed: protos (n, mh, mw, 32) and coef (n, max_det, 32) N(0, 1) (torch), boxes (n, max_det, 4)
    float32 (numpy; rows beyond the counts are zero), windows, ratio (None outside the default form)."""
    seed = case["seed"] if seed is None else seed
    (mh, mw), counts, md = case["grid"], case["counts"], case["max_det"]
    n = len(counts)
    protos = torch.randn(n, mh, mw, NM, generator=torch.Generator().manual_seed(seed))
    coef = torch.randn(n, md, NM, generator=torch.Generator().manual_seed(seed + 1))
    if case["mode"] == "default":
        ratio = (mw / case["in_hw"][1], mh / case["in_hw"][0])
        bw, bh = case["in_hw"][1], case["in_hw"][0]
    else:
        ratio = None
        bw, bh = case["out_hw"][1], case["out_hw"][0]
    rng = np.random.default_rng(seed)
    boxes = np.zeros((n, md, 4), np.float32)
    for b, k in enumerate(counts):
        d = case["degenerate"][1] if case["degenerate"] and case["degenerate"][0] == b else 0
        boxes[b, : k - d] = make_boxes(rng, k - d, bw, bh, ratio or (1.0, 1.0))
        boxes[b, k - d : k] = degenerate_boxes(bw, bh, ratio or (1.0, 1.0))[:d]
    windows = [tuple(case["window"] or (0, 0, mh, mw))] * n
    return dict(protos=protos, coef=coef, boxes=boxes, counts=list(counts), windows=windows, out_hw=tuple(case["out_hw"]), mode=case["mode"], ratio=ratio)


def _args(inp):
    return (inp["protos"], inp["coef"], inp["boxes"], inp["counts"], inp["windows"], inp["out_hw"], inp["mode"], inp["ratio"])


@lru_cache(maxsize=None)
def case_reference(tag):
    """(inputs, (ref, unsure, inbox)) of a case, computed once per process; callers leave the arrays unchanged."""
    inp = case_inputs(pm_case(tag))
    out = reference_masks(*_args(inp))
    for a in out:
        a.setflags(write=False)
    return inp, out
