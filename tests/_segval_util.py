"""The float64 reference of the segmentation validator's mask matching (``dy_val_mask_match``), shared by tools/make_segval_golden.py (which
records it next to the real reference's results in tests/golden/segval.npz) and by tests/test_segval_host.py / _gpu.py, which evaluate it
at run time.  Plain numpy and CPU torch; not collected.

Semantics (models/yolo/segment/val.py of the reference): ``ops.process_mask(upsample=False)`` = ``coef @ protos``, ``crop_mask`` with the
unscaled box times (mw / iw, mh / ih), ``> 0`` at prototype resolution; the overlap label map expanded to one mask per label, at ratio 2
its 2 x 2 replication; ``mask_iou`` in fp32 on the integer counts; ``match_predictions``.
"""
from __future__ import annotations

import numpy as np
import torch

from tests._mask_util import NM, UNSURE, degenerate_boxes, edges_clear, make_boxes

IOUV = np.linspace(0.5, 0.95, 10)


# ---- the restated match rule ---------------------------------------------------------------------------------------------------------
def match_rule(pred_cls, tcls, iou, iouv=IOUV):
    """best(d) = argmax_l m(l, d) (ties: lower l), biou(d) = max_l m(l, d), m = iou where the classes agree else 0;
    tp[d, t] = biou(d) >= t and no d' < d has best(d') == best(d) and biou(d') >= t.  iou: (L, D) fp32.  Returns (best, biou, tp);
    best = -1, biou = 0 without labels."""
    pred_cls, tcls = np.asarray(pred_cls), np.asarray(tcls)
    D, L = len(pred_cls), len(tcls)
    thr = np.asarray(iouv, np.float64).astype(np.float32)
    best, biou, tp = np.full(D, -1, np.int64), np.zeros(D, np.float32), np.zeros((D, len(thr)), bool)
    if L == 0:
        return best, biou, tp
    m = np.asarray(iou, np.float32) * (tcls[:, None] == pred_cls[None, :])
    best = m.argmax(0)  # (numpy: the first of equal maxima)
    biou = m[best, np.arange(D)].astype(np.float32)
    top = {}  # label -> largest biou among the higher-ranked detections whose best it is
    for d in range(D):
        prev = top.get(int(best[d]), np.float32(-1))
        tp[d] = (biou[d] >= thr) & ~(prev >= thr)
        top[int(best[d])] = max(prev, biou[d])
    return best, biou, tp


def has_tie(pred_cls, tcls, iou, lo=0.5):
    """A detection with two same-class labels at exactly the same IoU >= lo (the reference's order on such ties is not defined)."""
    m = np.asarray(iou, np.float32) * (np.asarray(tcls)[:, None] == np.asarray(pred_cls)[None, :])
    for d in range(m.shape[1]):
        col = m[:, d][m[:, d] >= lo]
        if len(col) != len(np.unique(col)):
            return True
    return False


def iou32(inter, area_gt, area_pred):
    """mask_iou's fp32 expression on the integer counts: inter (L, D), area_gt (L,), area_pred (D,)."""
    i, g, p = (np.asarray(a).astype(np.float32) for a in (inter, area_gt, area_pred))
    return i / (((g[:, None] + p[None, :]) - i) + np.float32(1e-7))


# ---- float64 evaluation of one image -------------------------------------------------------------------------------------------------
def expand_map(label_map, ratio):
    m = np.asarray(label_map).astype(np.int64)
    return np.repeat(np.repeat(m, ratio, 0), ratio, 1)


def pred_masks64(protos, coef, boxes, in_hw, *, crop_shift=0):
    """protos (mh, mw, 32), coef (k, 32), boxes (k, 4) fp32 -> (mask, unsure) bool (k, mh, mw).  The crop edges are the fp32 products the
    reference forms (box times fp32(mw / iw)).  ``crop_shift`` (mutation knob): the crop window moved by that many proto pixels."""
    p, c = np.asarray(protos, np.float64), np.asarray(coef, np.float64)
    mh, mw = p.shape[:2]
    v = np.einsum("nk,yxk->nyx", c, p)
    s = np.einsum("nk,yxk->nyx", np.abs(c), np.abs(p))
    b = np.asarray(boxes, np.float32)
    rx, ry = np.float32(mw / in_hw[1]), np.float32(mh / in_hw[0])
    with np.errstate(invalid="ignore", over="ignore"):
        x1, x2, y1, y2 = (b[:, 0] * rx).astype(np.float64) + crop_shift, (b[:, 2] * rx).astype(np.float64) + crop_shift, (b[:, 1] * ry).astype(np.float64), (b[:, 3] * ry).astype(np.float64)
        xs, ys = np.arange(mw)[None, None, :], np.arange(mh)[None, :, None]
        keep = (xs >= x1[:, None, None]) & (xs < x2[:, None, None]) & (ys >= y1[:, None, None]) & (ys < y2[:, None, None])
    return (v > 0) & keep, (np.abs(v) < UNSURE * s) & keep


def counts64(masks, label_map, nl, ratio, *, no_shift=False):
    """masks bool (k, mh, mw) -> inter (nl, k), area_pred (k,), area_gt (nl,) as int64.  ``no_shift`` (mutation knob): the ratio-2 labels read
    at [y, x] of the map (zero outside it) instead of [y >> 1, x >> 1]."""
    k, mh, mw = masks.shape
    if no_shift and ratio == 2:
        up = np.zeros((mh, mw), np.int64)
        gm = np.asarray(label_map).astype(np.int64)
        up[: gm.shape[0], : gm.shape[1]] = gm
    else:
        up = expand_map(label_map, ratio)
    inter = np.zeros((nl, k), np.int64)
    area_gt = np.zeros(nl, np.int64)
    for l in range(nl):
        g = up == l + 1
        area_gt[l] = g.sum()
        inter[l] = (masks & g[None]).sum((1, 2))
    return inter, masks.sum((1, 2)).astype(np.int64), area_gt


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def case_inputs(seed, grid, ratio, in_hw, max_det, counts, n_labels, nc=3, map_dtype=np.uint8, degenerate=None, one_pixel_labels=False,
                empty_label=False, empty_pred=False, single_cls=False):
    """A kernel case regenerated from its seed.  protos (B, mh, mw, 32), coef (B, max_det, 32) N(0, 1) (torch); boxes (B, max_det, 4) fp32 with
    clear crop edges; rows (B, max_det, 6) with descending confidence and random classes; per image a label map (gh, gw) and ``n_labels[b]``
    label classes.  Labels are painted from the float64 masks of random predictions (shifted by up to a pixel, later labels over earlier
    ones) so that the IoUs spread from 0 to 1.  ``degenerate`` = (image, how many of _mask_util.degenerate_boxes) fill that image's last rows."""
    mh, mw = grid
    gh, gw = mh // ratio, mw // ratio
    B = len(counts)
    rng = np.random.default_rng(seed)
    protos = torch.randn(B, mh, mw, NM, generator=torch.Generator().manual_seed(seed))
    # smoothed over the grid (5 x 5 box filter), so that the masks are blobs and a mask shifted by a pixel still overlaps its source
    protos = torch.nn.functional.avg_pool2d(protos.permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1).contiguous() * 5.0
    coef = torch.randn(B, max_det, NM, generator=torch.Generator().manual_seed(seed + 1))
    rat = (mw / in_hw[1], mh / in_hw[0])
    boxes = np.zeros((B, max_det, 4), np.float32)
    rows = np.zeros((B, max_det, 6), np.float32)
    maps = np.zeros((B, gh, gw), map_dtype)
    tcls, timg = [], []
    for b, k in enumerate(counts):
        dg = degenerate[1] if degenerate and degenerate[0] == b else 0
        if k - dg:
            boxes[b, : k - dg] = np.concatenate([make_boxes(rng, 1, in_hw[1], in_hw[0], rat) for _ in range(k - dg)], 0)  # (one by one: each redrawn on its own)
        if dg:
            boxes[b, k - dg : k] = degenerate_boxes(in_hw[1], in_hw[0], rat)[:dg]
        if empty_pred and k:
            boxes[b, 0] = [0.31, 0.27, 0.43, 0.39]  # narrower than a proto pixel and between two integer columns: empty crop
        rows[b, :k, :4] = boxes[b, :k]
        rows[b, :k, 4] = np.sort(rng.uniform(0.01, 0.99, k).astype(np.float32))[::-1]
        rows[b, :k, 5] = rng.integers(0, nc, k)
        nl = n_labels[b]
        cls = rng.integers(0, nc, nl).astype(np.float32)
        if one_pixel_labels:  # label l owns pixel l of the map, nothing else
            flat = maps[b].reshape(-1)
            flat[:nl] = np.arange(1, nl + 1)
        elif nl:
            m64 = pred_masks64(protos[b].numpy(), coef[b, :k].numpy(), boxes[b, :k], in_hw)[0] if k else np.zeros((0, mh, mw), bool)
            for l in range(nl):
                if k and l % 4 != 3:
                    d = int(rng.integers(0, k))
                    src = np.roll(m64[d], (int(rng.integers(-1, 2)), int(rng.integers(-1, 2))), (0, 1))[::ratio, ::ratio]
                    if rng.uniform() < 0.8:
                        cls[l] = rows[b, d, 5]
                else:
                    y0, x0 = int(rng.integers(0, gh)), int(rng.integers(0, gw))
                    src = np.zeros((gh, gw), bool)
                    src[y0 : y0 + max(gh // 3, 1), x0 : x0 + max(gw // 3, 1)] = True
                if empty_label and l == 0:
                    src = np.zeros((gh, gw), bool)  # owns no pixel at all
                maps[b][src] = l + 1
        tcls.append(cls), timg.append(np.full(nl, b, np.int32))
    return dict(protos=protos, coef=coef, boxes=boxes, rows=rows, counts=np.array(counts, np.int32), maps=maps, tcls=np.concatenate(tcls).astype(np.float32),
                timg=np.concatenate(timg).astype(np.int32), n_labels=list(n_labels), grid=(mh, mw), ratio=ratio, in_hw=tuple(in_hw), max_det=max_det,
                single_cls=single_cls, degenerate=degenerate)


def case_expected(c, *, crop_shift=0, no_shift=False, drop_class=False, no_eps=False):
    """Float64 evaluation of a case -> the kernel's outputs: inter (B, max_det, l_cap), area_pred (B, max_det), area_gt (B, l_cap), best_iou,
    best_label (position in tcls), tp_m, plus ``unsure`` (count of unsure in-crop pixels: the counts are exact iff 0), ``tie`` and per image
    the fp32 iou matrix.  The keyword knobs are the mutations of tests/test_segval_host.py."""
    B, md = len(c["counts"]), c["max_det"]
    l_cap = max(max(c["n_labels"]), 1)
    out = dict(inter=np.zeros((B, md, l_cap), np.int32), area_pred=np.zeros((B, md), np.int32), area_gt=np.zeros((B, l_cap), np.int32),
               best_iou=np.zeros((B, md), np.float32), best_label=np.full((B, md), -1, np.int32), tp_m=np.zeros((B, md, len(IOUV)), bool),
               unsure=0, tie=False, iou=[], l_cap=l_cap)
    off = 0
    for b, k in enumerate(c["counts"]):
        nl = c["n_labels"][b]
        tc = c["tcls"][off : off + nl]
        mask, uns = pred_masks64(c["protos"][b].numpy(), c["coef"][b, :k].numpy(), c["boxes"][b, :k], c["in_hw"], crop_shift=crop_shift)
        out["unsure"] += int(uns.sum())
        inter, ap, ag = counts64(mask, c["maps"][b], nl, c["ratio"], no_shift=no_shift)
        out["inter"][b, :k, :nl], out["area_pred"][b, :k], out["area_gt"][b, :nl] = inter.T, ap, ag
        iou = iou32(inter, ag, ap)
        if no_eps:
            with np.errstate(invalid="ignore", divide="ignore"):
                i, g, p = inter.astype(np.float32), ag.astype(np.float32), ap.astype(np.float32)
                iou = i / ((g[:, None] + p[None, :]) - i)
        pc = np.zeros(k, np.float32) if c["single_cls"] else c["rows"][b, :k, 5]
        tcm = tc  # (single_cls zeroes the predictions' class only, as dy_val_match and the host path do: the dataset's labels are class 0 then)
        if drop_class:
            pc, tcm = np.zeros(k, np.float32), np.zeros(nl, np.float32)
        best, biou, tp = match_rule(pc, tcm, iou)
        out["tie"] |= has_tie(pc, tcm, iou) if nl and k else False
        out["best_iou"][b, :k], out["tp_m"][b, :k] = biou, tp
        out["best_label"][b, :k] = np.where(best >= 0, best + off, -1)
        out["iou"].append(iou)
        off += nl
    return out


def edges_ok(c):
    """No crop edge of a non-degenerate kept row within 1e-2 of an integer (then the fp32 and float64 crop windows agree)."""
    mh, mw = c["grid"]
    rat = (mw / c["in_hw"][1], mh / c["in_hw"][0])
    for b, k in enumerate(c["counts"]):
        dg = c["degenerate"][1] if c["degenerate"] and c["degenerate"][0] == b else 0
        if k - dg and not edges_clear(c["boxes"][b, : k - dg], rat):
            return False
    return True
