"""Inputs of the oriented-box fixtures, shared by tools/make_obb_golden.py and the tests (not collected).  Everything is regenerated from a
seed (torch.Generator on the CPU); tests/golden/obb.npz stores the seed each case ended up with and what the reference returned."""
import math

import numpy as np
import torch

CONF, IOU, NC = 0.25, 0.45, 3
LDS_CAP = 2048  # dy_nms_rotated_lds_cap(); tests/test_obb_gpu.py asserts that the library says the same


def make_pred(counts, anchors, seed, nc=NC, wh=(2.0, 80.0), clusters=0, spread=600.0):
    """(pred (B, 4 + nc, anchors), theta (B, anchors)): exactly counts[b] anchors of image b have a best class score above CONF, all scores of an
    image distinct.  ``clusters``: boxes are jittered copies of that many objects, so most candidates are suppressed."""
    g = torch.Generator().manual_seed(seed)
    batch = len(counts)
    xy = torch.rand(batch, 2, anchors, generator=g) * spread + 20
    box_wh = torch.rand(batch, 2, anchors, generator=g) * (wh[1] - wh[0]) + wh[0]
    theta = (torch.rand(batch, anchors, generator=g) - 0.25) * math.pi
    if clusters:
        who = torch.randint(0, clusters, (batch, 1, anchors), generator=g)
        xy = torch.gather(xy[:, :, :clusters], 2, who.expand(batch, 2, anchors)) + torch.rand(batch, 2, anchors, generator=g) * 8
        box_wh = torch.gather(box_wh[:, :, :clusters], 2, who.expand(batch, 2, anchors)) + 30 + torch.rand(batch, 2, anchors, generator=g) * 8
        theta = torch.gather(theta[:, :clusters], 1, who[:, 0]) + (torch.rand(batch, anchors, generator=g) - 0.5) * 0.2
    sc = torch.rand(batch, nc, anchors, generator=g) * 0.2  # nobody clears CONF ...
    for b, n in enumerate(counts):
        who = torch.randperm(anchors, generator=g)[:n]  # ... but these n anchors, in one random class each
        cls = torch.randint(0, nc, (n,), generator=g)
        sc[b, cls, who] = 0.3 + 0.7 * (torch.randperm(n, generator=g).float() + 0.5) / max(n, 1)
    return torch.cat((xy, box_wh, sc), 1).contiguous(), theta.contiguous()


def _set(pred, theta, b, a, box, score, cls):
    pred[b, :4, a] = torch.tensor(box[:4], dtype=torch.float32)
    pred[b, 4:, a] = 0.01
    pred[b, 4 + cls, a] = score
    theta[b, a] = box[4]


def chain_boxes(d):
    """A, B, C in a row, ``d`` apart: A overlaps B, B overlaps C, A does not overlap C (at the IoU threshold)."""
    return [(100.0, 100.0, 60.0, 24.0, 0.3), (100.0 + d * math.cos(0.3), 100.0 + d * math.sin(0.3), 60.0, 24.0, 0.3),
            (100.0 + 2 * d * math.cos(0.3), 100.0 + 2 * d * math.sin(0.3), 60.0, 24.0, 0.3)]


CHAIN_D = 22.0

# name -> (counts, anchors, make_pred keywords, keywords of the NMS call, what the case is for)
NMS_CASES = {
    "few": ([0, 1, 2], 64, {}, {}, "no candidate, one, and two identical ones (box, angle, class AND score: the lower anchor wins)"),
    "chunks": ([63, 64, 65, 129], 256, dict(clusters=12), {}, "candidate counts around the chunk size of 64"),
    "lds_cap": ([LDS_CAP + 200, 300], LDS_CAP + 512, dict(clusters=40), {}, "one image over the LDS table capacity and one under it in the same batch"),
    "crowd": ([400, 30], 512, dict(wh=(2.0, 6.0)), dict(max_det=50), "more kept than max_det: the scan stops"),
    "max_nms": ([300, 100], 512, dict(clusters=20), dict(max_nms=128), "the max_nms truncation"),
    "same_place": ([40], 64, dict(clusters=4), {}, "same place, different classes: kept apart by the class offset"),
    "same_place_agnostic": ([40], 64, dict(clusters=4), dict(agnostic=True), "the same input without the class offset"),
    "class_mask": ([200, 90], 256, dict(clusters=16), dict(classes=[0, 2]), "a class filter"),
    "degenerate": ([80], 128, dict(clusters=6), {}, "zero-width and zero-height boxes among the candidates"),
    "chain": ([3], 64, {}, {}, "fast versus greedy: A suppresses B, B alone overlaps C; the reference drops C, a greedy scan keeps it"),
}


def nms_inputs(name, seed):
    counts, anchors, mk, _, _ = NMS_CASES[name]
    if name == "chain":
        pred, theta = make_pred([0], anchors, seed)
        for k, box in enumerate(chain_boxes(CHAIN_D)):
            _set(pred, theta, 0, 5 + 7 * k, box, 0.9 - 0.1 * k, 1)
        return pred, theta
    pred, theta = make_pred(counts, anchors, seed, **mk)
    if name == "few":
        pred, theta = make_pred([0, 1, 0], anchors, seed)
        for a in (9, 41):
            _set(pred, theta, 2, a, (200.0, 120.0, 40.0, 16.0, 0.7), 0.625, 2)
    if name == "degenerate":
        cand = (pred[0, 4:].amax(0) > CONF).nonzero()[:, 0]
        pred[0, 2, cand[:6]] = 0.0    # zero width
        pred[0, 3, cand[6:12]] = 0.0  # zero height
    return pred, theta


def candidate_counts(pred, kw):
    best, j = pred[:, 4:].max(1)
    ok = best > CONF
    if kw.get("classes") is not None:
        ok &= torch.isin(j, torch.tensor(kw["classes"]))
    return ok.sum(1).tolist()


def probiou64(boxes):
    """(n, n) ProbIoU of xywhr ``boxes`` (n, 5) in float64 numpy: batch_probiou's expression (reference utils/metrics.py:244-275)."""
    b = np.asarray(boxes, np.float64)
    x, y = b[:, 0], b[:, 1]
    a_, b_ = b[:, 2] ** 2 / 12, b[:, 3] ** 2 / 12
    cos, sin = np.cos(b[:, 4]), np.sin(b[:, 4])
    a, bb, c = a_ * cos**2 + b_ * sin**2, a_ * sin**2 + b_ * cos**2, (a_ - b_) * cos * sin
    sa, sb, sc = a[:, None] + a[None], bb[:, None] + bb[None], c[:, None] + c[None]
    dx, dy = x[:, None] - x[None], y[:, None] - y[None]
    eps = 1e-7
    det = sa * sb - sc**2
    t1 = (sa * dy**2 + sb * dx**2) / (det + eps) * 0.25
    t2 = (sc * (-dx) * dy) / (det + eps) * 0.5
    d = np.clip(a * bb - c**2, 0, None)
    with np.errstate(invalid="ignore"):  # (a degenerate pair's determinant can round below zero: NaN, as in the reference)
        t3 = np.log(det / (4 * np.sqrt(d[:, None] * d[None]) + eps) + eps) * 0.5
    bd = np.clip(t1 + t2 + t3, eps, 100.0)
    return 1 - np.sqrt(1.0 - np.exp(-bd) + eps)


def sorted_candidates(pred, theta, b, kw, max_wh=7680.0):
    """The candidates of image b as the NMS sees them: (anchors in score order after max_nms, xywhr boxes WITH the class offset in fp32, scores)."""
    best, j = pred[b, 4:].max(0)
    ok = best > CONF
    if kw.get("classes") is not None:
        ok &= torch.isin(j, torch.tensor(kw["classes"]))
    idx = ok.nonzero()[:, 0]
    order = torch.sort(best[idx], descending=True, stable=True).indices[: kw.get("max_nms", 30000)]
    idx = idx[order]
    c = j[idx].float() * (0.0 if kw.get("agnostic") else max_wh)
    boxes = torch.stack((pred[b, 0, idx] + c, pred[b, 1, idx] + c, pred[b, 2, idx], pred[b, 3, idx], theta[b, idx]), 1)
    return idx, boxes, best[idx]


def fast_nms(iou, thr):
    """Kept positions of the reference's fast NMS on an (n, n) IoU matrix in score order."""
    return [j for j in range(iou.shape[0]) if not (iou[:j, j] >= thr).any()]


def greedy_nms(iou, thr):
    kept = []
    for j in range(iou.shape[0]):
        if not any(iou[i, j] >= thr for i in kept):
            kept.append(j)
    return kept


# ---- dy_obb_decode ---------------------------------------------------------------------------------------------------------------
DECODE_LEVELS = ((6, 10, 4.0, 4), (3, 5, 8.0, 8), (2, 2, 16.0, 4), (1, 1, 32.0, 8))  # h, w, stride, pitch of the angle map
DECODE_BATCH, DECODE_NC = 3, 2


def decode_inputs(seed):
    """(lt, rb distances (B, 4, A) in grid units, angle logits per level [(B, h, w)], anchors (A, 2) in grid units, strides (A,)).
    The first and last anchor of every level get the logits -30 / +30 (image 0), +30 / -30 (image 1) and 0 / 0 (image 2)."""
    g = torch.Generator().manual_seed(seed)
    A = sum(h * w for h, w, _, _ in DECODE_LEVELS)
    dist = torch.rand(DECODE_BATCH, 4, A, generator=g) * 6 + 0.1
    logits, anchors, strides = [], [], []
    for h, w, s, _ in DECODE_LEVELS:
        lg = torch.randn(DECODE_BATCH, h, w, generator=g) * 2
        lg.view(DECODE_BATCH, -1)[0, [0, -1]] = torch.tensor([-30.0, 30.0])
        lg.view(DECODE_BATCH, -1)[1, [0, -1]] = torch.tensor([30.0, -30.0])
        lg.view(DECODE_BATCH, -1)[2, [0, -1]] = 0.0
        logits.append(lg)
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing="ij")
        anchors.append(torch.stack((xx.reshape(-1), yy.reshape(-1)), 1))
        strides.append(torch.full((h * w,), s))
    return dist, logits, torch.cat(anchors), torch.cat(strides)


def detect_xywh(dist, anchors, strides):
    """What Detect's decode leaves in rows 0..3 of pred (dist2bbox, xywh, times the stride), in the precision of ``dist``."""
    a = anchors.to(dist.dtype).t()[None]
    lt, rb = dist[:, :2], dist[:, 2:]
    x1y1, x2y2 = a - lt, a + rb
    return torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), 1) * strides.to(dist.dtype)[None, None]
