"""Inputs and float64 restatements of the oriented-box validation fixtures, shared by tools/make_obbval_golden.py and the tests (not
collected).  Everything is regenerated from a seed; tests/golden/obbval.npz stores the seed each case ended up with, the margins measured on
it and what the reference returned.

The margin rule: every same-class (label, detection) pair is evaluated in float64 and in fp32; M = 8 x max |iou32 - iou64| over
the pairs whose float64 value lies in [0.4, 0.97] (the band that can decide a threshold), M_top the same over the pairs above 0.97, where
ProbIoU is ill-conditioned.  A seed is a fixture only if no same-class pair lies within M of a threshold, no detection that can reach 0.5 has
its two best same-class labels within M of each other, no NaN stands where a decision is made, and the float64 rule, the fp32
``match_predictions`` and the recorded ``tp`` agree."""
import math

import numpy as np
import torch

from tests import _obb_util as U

IOUV = np.linspace(0.5, 0.95, 10)
BAND_LO, BAND_HI = 0.4, 0.97
NC = 3
CONF, IOU = U.CONF, U.IOU
MAX_WH = 7680.0


def probiou64(a, b):
    """(n, m) float64 ProbIoU of xywhr boxes a (n, 5) against b (m, 5): tests/_obb_util.py::probiou64 on the two sets together."""
    a, b = np.asarray(a, np.float64).reshape(-1, 5), np.asarray(b, np.float64).reshape(-1, 5)
    return U.probiou64(np.concatenate((a, b)))[: len(a), len(a) :]


def clip_xywhr(boxes, w, h):
    """scale_boxes(xywh=True) at gain 1, pad 0 = clip_boxes on xywh rows, in fp32: columns 0 and 2 to [0, w], 1 and 3 to [0, h]."""
    out = np.array(boxes, np.float32, copy=True)
    out[:, [0, 2]] = out[:, [0, 2]].clip(0, w)
    out[:, [1, 3]] = out[:, [1, 3]].clip(0, h)
    return out


# ---- dy_val_match_rotated: kernel-free cases -------------------------------------------------------------------------------------------
# name -> keywords of _gen (counts: detections per image, nlab: labels per image)
MATCH_CASES = {
    "val300": dict(max_det=300, counts=[300, 37], nlab=[40, 12], clip=(640, 512)),  # (first: its margins are the floor of the others')
    "few": dict(max_det=8, counts=[0, 1, 5], nlab=[3, 0, 4], clip=(160, 128)),
    "rank": dict(max_det=4, counts=[2], nlab=[2], clip=(320, 256)),
    "step": dict(max_det=16, counts=[16, 9], nlab=[300, 230], clip=(1280, 1024)),
    "stride": dict(max_det=520, counts=[520, 3], nlab=[40, 6], clip=(640, 512)),
    "clip": dict(max_det=16, counts=[12, 10], nlab=[6, 5], clip=(160, 128), outside=True),
    "angles": dict(max_det=16, counts=[14], nlab=[10], clip=(320, 256), swap=4),
    "degenerate": dict(max_det=8, counts=[7], nlab=[5], clip=(320, 256), degenerate=True),
}
SINGLE_CLS_OF = "few"  # the `single_cls` case: these inputs with every label's class 0 and single_cls=True (one seed serves both)


def _gen(seed, max_det, counts, nlab, clip, outside=False, swap=0, degenerate=False):
    rng = np.random.default_rng(seed)
    W, H = clip
    B = len(counts)
    rows = (rng.standard_normal((B, max_det, 7)) * 1e3).astype(np.float32)  # garbage beyond the counts
    tbox, tcls, timg = [], [], []
    for i, (cnt, nl) in enumerate(zip(counts, nlab)):
        lb = np.stack((rng.uniform(0.1 * W, 0.9 * W, nl), rng.uniform(0.1 * H, 0.9 * H, nl), rng.uniform(8, 60, nl), rng.uniform(6, 40, nl),
                       rng.uniform(-math.pi / 4, 3 * math.pi / 4, nl)), 1)
        lc = rng.integers(0, NC, nl).astype(np.float32)
        if outside and nl >= 4:
            lb[0, 0], lb[1, 1] = -7.0, H + 9.0          # centres outside the image
            lb[2, 2], lb[3, 3] = 2.5 * W, 1.5 * H       # wider / taller than the image
        if degenerate and nl >= 2:
            lb[0, 2] = 0.0                               # a zero-width label
        if cnt:
            if nl:
                src = rng.integers(0, nl, cnt)
                src[: min(cnt, nl)] = np.arange(min(cnt, nl))  # every label has a detection of its own
                u = rng.random(cnt) ** 2
                pb = lb[src].copy()
                pb[:, :2] += rng.normal(0, 1, (cnt, 2)) * u[:, None] * 12
                pb[:, 2:4] *= 1 + np.abs(rng.normal(0, 1, (cnt, 2))) * u[:, None] * 0.5
                pb[:, 4] += rng.normal(0, 1, cnt) * u * 0.5
                pc = lc[src].copy()
                flip = rng.random(cnt) < 0.15
                pc[flip] = (pc[flip] + rng.integers(1, NC, int(flip.sum()))) % NC
                order = rng.permutation(cnt)
                pb, pc, src = pb[order], pc[order], src[order]
                for k in range(min(swap, cnt)):  # the same box written the other way: (w, h, theta) <-> (h, w, theta + pi / 2)
                    l = lb[src[k]]
                    pb[k] = (l[0], l[1], l[3], l[2], l[4] + math.pi / 2 if l[4] < math.pi / 4 else l[4] - math.pi / 2)
                    pc[k] = lc[src[k]]
                if degenerate:
                    pb[src == 0, 2] = 20.0  # (the copies of the zero-width label have a width: two parallel degenerate boxes have no defined ProbIoU)
                    pb[0, 3] = 0.0          # a zero-height detection
            else:
                pb = np.stack((rng.uniform(0, W, cnt), rng.uniform(0, H, cnt), rng.uniform(8, 60, cnt), rng.uniform(6, 40, cnt), rng.uniform(-0.7, 2.3, cnt)), 1)
                pc = rng.integers(0, NC, cnt).astype(np.float32)
            rows[i, :cnt, :5] = pb
            rows[i, :cnt, 5] = np.sort(rng.uniform(0.001, 1, cnt))[::-1]
            rows[i, :cnt, 6] = pc
        tbox.append(lb), tcls.append(lc), timg.append(np.full(nl, i))
    tbox = clip_xywhr(np.concatenate(tbox).astype(np.float32), W, H)  # what _prepare_batch leaves
    tcls, timg = np.concatenate(tcls), np.concatenate(timg).astype(np.int32)
    perm = rng.permutation(len(tbox))  # batch layout: labels belong to images by value, in no order
    return dict(rows=rows, counts=np.array(counts, np.int32), tbox=tbox[perm], tcls=tcls[perm], timg=timg[perm], clip=(W, H), max_det=max_det, single_cls=False)


def _rank_case():
    """Two detections whose best label is the same one; the higher-ranked detection has the LOWER IoU (0.818 against 0.949)."""
    lab = np.array([[100.0, 100.0, 60.0, 24.0, 0.3], [220.0, 180.0, 40.0, 30.0, 1.9]], np.float32)
    rows = np.full((1, 4, 7), 9e5, np.float32)
    rows[0, 0] = (100.0 + 9.0 * math.cos(0.3), 100.0 + 9.0 * math.sin(0.3), 60.0, 24.0, 0.3, 0.9, 1.0)
    rows[0, 1] = (100.0 + 2.5 * math.cos(0.3), 100.0 + 2.5 * math.sin(0.3), 60.0, 24.0, 0.3, 0.8, 1.0)
    return dict(rows=rows, counts=np.array([2], np.int32), tbox=lab, tcls=np.array([1.0, 1.0], np.float32), timg=np.zeros(2, np.int32), clip=(320, 256),
                max_det=4, single_cls=False)


def match_inputs(name, seed):
    if name == "rank":
        return _rank_case()
    if name == "single_cls":
        c = _gen(seed, **MATCH_CASES[SINGLE_CLS_OF])
        c["tcls"] = np.zeros_like(c["tcls"])  # (what single_cls makes of a dataset: every label is class 0)
        c["single_cls"] = True
        return c
    return _gen(seed, **MATCH_CASES[name])


def _grid_labels(n, pitch=60.0):
    """n 20 x 10 boxes of mixed angles on a grid ``pitch`` px apart: every pair of different boxes scores below 0.01."""
    i = np.arange(n)
    return np.stack((40.0 + pitch * (i % 17), 40.0 + pitch * (i // 17), np.full(n, 20.0), np.full(n, 10.0), (i % 7) * 0.4 - 0.7), 1).astype(np.float32)


def full_stage_case():
    """A stage filled exactly to capacity: 257 labels of one class, all of image 0 and in order (the first step stages 256 entries, the second
    one); detections = exact copies of labels 0, 255 and 256, and a second copy of label 256 ranked below the first.  No seed: every same-class
    pair is above 0.99 or below 0.01."""
    lab = _grid_labels(257)
    rows = np.zeros((1, 4, 7), np.float32)
    rows[0, :, :5] = lab[[0, 255, 256, 256]]
    rows[0, :, 5], rows[0, :, 6] = (0.9, 0.8, 0.7, 0.6), 1.0
    return dict(rows=rows, counts=np.array([4], np.int32), tbox=lab, tcls=np.ones(257, np.float32), timg=np.zeros(257, np.int32), clip=(1100, 1040),
                max_det=4, single_cls=False)


def bound_case():
    """The LDS layout at its upper bound: max_det 4096, all rows kept, 5 labels.  The first five detections are copies of the labels, the rest
    far-away boxes of a class no label has."""
    lab = _grid_labels(5)
    rng = np.random.default_rng(0)
    rows = np.zeros((1, 4096, 7), np.float32)
    rows[0, :, :5] = np.stack((rng.uniform(500, 1000, 4096), rng.uniform(500, 1000, 4096), rng.uniform(8, 60, 4096), rng.uniform(6, 40, 4096),
                               rng.uniform(-0.7, 2.3, 4096)), 1)
    rows[0, :, 5], rows[0, :, 6] = np.linspace(0.99, 0.01, 4096), 2.0
    rows[0, :5, :5], rows[0, :5, 6] = lab, (0.0, 1.0, 0.0, 1.0, 0.0)
    return dict(rows=rows, counts=np.array([4096], np.int32), tbox=lab, tcls=np.array([0.0, 1.0, 0.0, 1.0, 0.0], np.float32), timg=np.zeros(5, np.int32),
                clip=(1100, 1040), max_det=4096, single_cls=False)


def expect64(c):
    """``rule64`` on a one-image case whose labels are in image order: tp (max_det, T), best_label (max_det,), and the float64 scores of the
    same-class pairs."""
    cnt = int(c["counts"][0])
    i64 = probiou64(c["tbox"], clip_xywhr(c["rows"][0, :cnt, :5], *c["clip"]))
    same = c["tcls"][:, None] == c["rows"][0, :cnt, 6][None]
    tp, best, _ = rule64(np.where(same, i64, 0.0))
    return tp, best, i64[same]


def rule64(m, iouv=IOUV):
    """The restated match rule on a class-masked (L, D) matrix (NaN: never the best): tp (D, T) bool, best (D,) position among the L labels
    (-1: none), biou (D,)."""
    L, D = m.shape
    tp = np.zeros((D, len(iouv)), bool)
    if L == 0 or D == 0:
        return tp, np.full(D, -1, np.int64), np.zeros(D)
    mm = np.where(np.isnan(m), -np.inf, m)
    best, biou = mm.argmax(0), mm.max(0)  # (the first maximum: ties go to the lower position)
    best = np.where(np.isfinite(biou), best, -1)
    prev, seen = np.full(D, -np.inf), {}
    for d in range(D):  # prev(d): the largest biou of a higher-ranked detection with the same best label
        if best[d] >= 0:
            prev[d] = seen.get(int(best[d]), -np.inf)
            seen[int(best[d])] = max(prev[d], biou[d])
    thr = np.asarray(iouv)[None]
    tp = (best >= 0)[:, None] & (biou[:, None] >= thr) & ~(prev[:, None] >= thr)
    return tp, best, np.where(best >= 0, biou, 0.0)


def match_evaluate(c, probiou32, match32, rows64=None, floor=(0.0, 0.0), fixed=None):
    """Evaluates a case in float64 and in fp32 (``probiou32(gt (L, 5), det (D, 5)) -> (L, D)`` fp32 array, ``match32(pred_cls, true_cls, iou)
    -> (D, T)`` bool: the reference's functions in the builder, this package's restatements in the tests).  Returns M, M_top, the float64
    tp / best_iou / best_label (batch layout, label positions in tbox), the fp32 tp and ``ok``: the acceptance conditions.  ``rows64``: the
    float64 side's own detections (the rows of a float64 model run) instead of ``c["rows"]``.  ``floor``: (M, M_top) of the ``val300`` case
    (300 detections x 40 labels, the validator's load): a case of a handful of pairs does not sample the fp32 error of the expression, so its
    margins are never taken below those -- a larger margin makes the acceptance conditions stricter.  ``fixed``: (M, M_top) to judge the
    conditions with (the tests: the recorded margins; fp32 sin / cos / log / exp of another CPU differ in the last bit, so the margins
    re-measured there are not bit-equal to the recorded ones; ``M_meas`` / ``M_top_meas`` are what this call measured)."""
    B, md = len(c["counts"]), c["max_det"]
    W, H = c["clip"]
    tp64, tp32 = np.zeros((B, md, len(IOUV)), bool), np.zeros((B, md, len(IOUV)), bool)
    biou64, best64 = np.zeros((B, md)), np.full((B, md), -1, np.int64)
    d_band, d_top, per_image = 0.0, 0.0, []
    for i, cnt in enumerate(c["counts"]):
        where = np.nonzero(c["timg"] == i)[0]
        if cnt == 0 or len(where) == 0:
            continue
        det = clip_xywhr(c["rows"][i, :cnt, :5], W, H)
        pcls = np.zeros(cnt, np.float32) if c["single_cls"] else c["rows"][i, :cnt, 6]
        lab, lcls = c["tbox"][where], c["tcls"][where]
        with np.errstate(all="ignore"):
            det64 = det
            if rows64 is not None:
                det64 = np.array(rows64[i, :cnt, :5], np.float64)
                det64[:, [0, 2]], det64[:, [1, 3]] = det64[:, [0, 2]].clip(0, W), det64[:, [1, 3]].clip(0, H)
            i64 = probiou64(lab, det64)
            i32 = np.asarray(probiou32(lab, det), np.float32).astype(np.float64)
        same = lcls[:, None] == pcls[None]
        per_image.append((i64, i32, same))
        band = same & (i64 >= BAND_LO) & (i64 <= BAND_HI)
        top = same & (i64 > BAND_HI)
        if band.any():
            d_band = max(d_band, float(np.abs(i32 - i64)[band].max()))
        if top.any():
            d_top = max(d_top, float(np.abs(i32 - i64)[top].max()))
        t, b, v = rule64(np.where(same, i64, 0.0))
        tp64[i, :cnt], biou64[i, :cnt], best64[i, :cnt] = t, v, np.where(b >= 0, where[np.maximum(b, 0)], -1)
        tp32[i, :cnt] = match32(pcls, lcls, np.asarray(probiou32(lab, det), np.float32))
    M, M_top = (max(8 * d_band, floor[0]), max(8 * d_top, floor[1])) if fixed is None else fixed
    ok, near = True, np.inf
    for i64, i32, same in per_image:
        n64, n32 = np.isnan(i64) & same, np.isnan(i32) & same
        # a NaN may stand only where the other precision is NaN too or far below every threshold
        ok &= not (n64 & ~n32 & (i32 >= BAND_LO)).any() and not (n32 & ~n64 & (i64 >= BAND_LO)).any()
        v = np.where(same & ~np.isnan(i64), i64, -1.0)
        tol = np.where(v > BAND_HI, M_top, M)
        dist = np.abs(v[:, :, None] - IOUV[None, None])
        ok &= not (dist <= tol[:, :, None])[v >= 0].any()  # no pair within the margin of a threshold
        near = min(near, float(dist[v >= 0].min(initial=np.inf)))
        if v.shape[0] > 1:
            top2 = np.sort(v, 0)[-2:]
            tie = (top2[1] >= 0.5 - M) & (top2[1] - top2[0] <= np.where(top2[1] > BAND_HI, M_top, M))
            ok &= not tie.any()  # the two best same-class labels of a detection that can reach 0.5 are apart
    ok &= bool(np.array_equal(tp64, tp32))
    return dict(M=M, M_top=M_top, tp64=tp64, tp32=tp32, best_iou64=biou64, best_label64=best64, ok=bool(ok), near=near, M_meas=8 * d_band, M_top_meas=8 * d_top)


# ---- dy_nms_rotated_ml -----------------------------------------------------------------------------------------------------------------
# name -> (pairs above conf per image, anchors, nc, make_pred_ml keywords, keywords of the NMS call, what the case is for)
NMS_CASES = {
    "two": ([2, 9], 64, 3, {}, {}, "two classes above conf on one anchor: both survive (the class offset keeps them apart)"),
    "two_agnostic": ([2, 9], 64, 3, {}, dict(agnostic=True), "the same input without the class offset: the lower-scored one falls"),
    "chunks": ([63, 64, 65, 129], 128, 3, dict(clusters=12), {}, "candidate counts, in (anchor, class) pairs, around the chunk size of 64"),
    "lds_cap": ([U.LDS_CAP + 200, 300], 1024, 3, dict(clusters=40), {}, "over the LDS table capacity BECAUSE of multi_label: anchors below it, pairs above"),
    "max_nms": ([300, 100], 256, 3, dict(clusters=20), dict(max_nms=128), "the max_nms truncation"),
    "crowd": ([400, 30], 256, 3, dict(wh=(2.0, 6.0)), dict(max_det=50), "more kept than max_det: the scan stops"),
    "nc1": ([90, 40], 128, 1, dict(clusters=10), {}, "nc = 1: the single-label form, identical to nms_rotated"),
}


def make_pred_ml(counts, anchors, seed, nc, wh=(2.0, 80.0), clusters=0, spread=600.0):
    """(pred (B, 4 + nc, anchors), theta (B, anchors)): exactly counts[b] (anchor, class) pairs of image b score above CONF, spread over the
    anchors at random so that many anchors carry several; all scores of an image are distinct."""
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
        pair = torch.randperm(anchors * nc, generator=g)[:n]  # ... but these n (anchor, class) pairs
        sc[b, pair % nc, pair // nc] = 0.3 + 0.7 * (torch.randperm(n, generator=g).float() + 0.5) / max(n, 1)
    return torch.cat((xy, box_wh, sc), 1).contiguous(), theta.contiguous()


def nms_inputs(name, seed):
    counts, anchors, nc, mk, _, _ = NMS_CASES[name]
    if name.startswith("two"):
        pred, theta = make_pred_ml([0, counts[1]], anchors, seed, nc)
        pred[0, :4, 17] = torch.tensor([200.0, 120.0, 40.0, 16.0])
        theta[0, 17] = 0.7
        pred[0, 4:, 17] = torch.tensor([0.8, 0.1, 0.6])  # classes 0 and 2 of anchor 17
        return pred, theta
    return make_pred_ml(counts, anchors, seed, nc, **mk)


def pair_counts(pred, nc):
    return (pred[:, 4 : 4 + nc] > CONF).sum((1, 2)).tolist()


def ml_sorted_candidates(pred, theta, b, nc, kw, conf=CONF):
    """The candidates of image b as the multi_label NMS sees them: (anchors, classes, xywhr boxes WITH the class offset in fp32, scores), in
    score order (ties: ascending anchor * nc + class, the row-major order of torch.where) after the max_nms cut."""
    sc = pred[b, 4 : 4 + nc].t().contiguous()  # (A, nc)
    a, c = torch.where(sc > conf)
    s = sc[a, c]
    order = torch.sort(s, descending=True, stable=True).indices[: kw.get("max_nms", 30000)]
    a, c, s = a[order], c[order], s[order]
    off = c.float() * (0.0 if kw.get("agnostic") else MAX_WH)
    boxes = torch.stack((pred[b, 0, a] + off, pred[b, 1, a] + off, pred[b, 2, a], pred[b, 3, a], theta[b, a]), 1)
    return a, c, boxes, s


def nms_evaluate(pred, theta, nc, kw, probiou32, conf=CONF, iou=IOU, floor=0.0, fixed=None):
    """The robust-verdict condition on one NMS input.  Returns (ok, M, kept positions per image from the float64 matrix).  ``floor``: the
    margin is not taken below it (the end-to-end fixtures: the rows of another implementation of the model differ by more than fp32 ProbIoU does)."""
    worst, mats = 0.0, []
    for b in range(pred.shape[0]):
        _, _, boxes, s = ml_sorted_candidates(pred, theta, b, nc, kw, conf)
        if len(s) != len(torch.unique(s)):
            return False, 0.0, []
        if len(boxes) < 2:
            mats.append(np.zeros((len(boxes), len(boxes))))
            continue
        bx = boxes.numpy()
        with np.errstate(all="ignore"):
            i64 = U.probiou64(bx)
            i32 = np.asarray(probiou32(bx, bx), np.float32).astype(np.float64)
        up = np.triu(np.ones_like(i64, bool), 1)
        if np.isnan(i32[up]).any() or np.isnan(i64[up]).any():
            return False, 0.0, []
        worst = max(worst, float(np.abs(i32 - i64)[up].max()))
        mats.append(i64)
    M = max(8 * worst, floor) if fixed is None else max(fixed, 8 * worst)  # (fixed: the recorded margin, see match_evaluate)
    if float((pred[:, 4 : 4 + nc] - conf).abs().min()) <= 8 * worst:
        return False, M, []
    kept = []
    for i64 in mats:
        n = i64.shape[0]
        k = []
        for j in range(n):
            col = i64[:j, j]
            if (col >= iou + M).any():
                continue  # robustly suppressed
            if (col < iou - M).all():
                k.append(j)  # robustly kept
                continue
            return False, M, []
        kept.append(k)
    return True, M, kept


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
E2E = {  # tag -> (yaml, images, batch)
    "ov3": ("yolov8-obb.yaml", 4, 3),
    "ovp2": ("yolov8-p2-repvgg-obb.yaml", 3, 2),
}
E2E_HW, E2E_NC = (64, 96), 10


def e2e_images(seed, n):
    return torch.randint(0, 256, (n, 3, *E2E_HW), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
