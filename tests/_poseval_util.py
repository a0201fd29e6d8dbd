"""Inputs and float64 restatements of the pose validation fixtures, shared by tools/make_poseval_golden.py and the tests (not collected).
Everything is regenerated from a seed; tests/golden/poseval.npz stores the seed each case ended up with, the margin measured on it and what
the reference returned.

The margin rule (as §21's): every same-class (label, detection) pair is evaluated in float64 and in fp32; M = 8 x max |oks32 -
oks64| over the pairs whose float64 value is at least 0.4 (the band that can decide a threshold).  A seed is a fixture only if no same-class
pair lies within M of a threshold, no detection that can reach 0.5 has its two best same-class labels within M of each other, and the float64
rule, the fp32 ``match_predictions`` and the recorded ``tp`` agree."""
import numpy as np
import torch

from tests._obbval_util import rule64  # the restated match rule on a class-masked (L, D) matrix: task-independent

IOUV = np.linspace(0.5, 0.95, 10)
BAND_LO = 0.4
NC = 3
COCO_SIGMA = np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89]) / 10.0
STAGE = 64  # labels per step of dy_val_oks_match (csrc/val_oks.hip: OKS_STEP)
THREADS = 512


def sigma_of(kpt_shape):
    """PoseValidator.init_metrics: the COCO constants for [17, 3], ones(nkpt) / nkpt otherwise."""
    return COCO_SIGMA if list(kpt_shape) == [17, 3] else np.ones(kpt_shape[0]) / kpt_shape[0]


def clip_kpts(k, w, h):
    """ops.scale_coords at gain 1, pad 0 = clip_coords, in the array's precision: x to [0, w], y to [0, h]; further columns untouched."""
    out = np.array(k, copy=True)
    out[..., 0] = out[..., 0].clip(0, w)
    out[..., 1] = out[..., 1].clip(0, h)
    return out


def oks64(tbox, tkpt, pk, sigma):
    """(L, D) float64 object keypoint similarity: kpt_iou (utils/metrics.py:156-175) with area = box area * 0.53, every step in float64 on
    the given values.  tbox (L, 4) xyxy, tkpt (L, nkpt, 3), pk (D, nkpt, >= 2) clipped predictions."""
    tbox, tkpt, pk = np.asarray(tbox, np.float64), np.asarray(tkpt, np.float64), np.asarray(pk, np.float64)
    area = (tbox[:, 2] - tbox[:, 0]) * (tbox[:, 3] - tbox[:, 1]) * 0.53
    d = (tkpt[:, None, :, 0] - pk[None, :, :, 0]) ** 2 + (tkpt[:, None, :, 1] - pk[None, :, :, 1]) ** 2
    mask = tkpt[..., 2] != 0
    with np.errstate(all="ignore"):
        e = d / ((2 * np.asarray(sigma, np.float64)) ** 2 * (area[:, None, None] + 1e-7) * 2)
        return (np.exp(-e) * mask[:, None]).sum(-1) / (mask.sum(-1)[:, None] + 1e-7)


# ---- dy_val_oks_match: kernel-free cases -----------------------------------------------------------------------------------------------
# name -> keywords of _gen (counts: detections per image, nlab: labels per image)
MATCH_CASES = {
    "val300": dict(max_det=300, counts=[300, 37], nlab=[40, 12], clip=(640, 512)),  # (first: its margin is the floor of the others')
    "few": dict(max_det=8, counts=[0, 1, 5], nlab=[3, 0, 4], clip=(160, 128)),
    "rank": dict(max_det=4, counts=[2], nlab=[2], clip=(320, 256)),
    "step": dict(max_det=16, counts=[16, 9], nlab=[80, 50], clip=(1280, 1024)),
    "stride": dict(max_det=520, counts=[520, 3], nlab=[40, 6], clip=(640, 512)),
    "clip": dict(max_det=16, counts=[12, 10], nlab=[6, 5], clip=(160, 128), outside=True),
    "invisible": dict(max_det=16, counts=[14, 6], nlab=[8, 3], clip=(320, 256), invisible=True),
    "zero_area": dict(max_det=8, counts=[7], nlab=[5], clip=(320, 256), zero_area=True),
    "kpt4x2": dict(max_det=16, counts=[13, 4], nlab=[7, 3], clip=(320, 256), kpt_shape=(4, 2)),
}
SINGLE_CLS_OF = "few"  # the `single_cls` case: these inputs with every label's class 0 and single_cls=True (one seed serves both)


def _gen(seed, max_det, counts, nlab, clip, kpt_shape=(17, 3), outside=False, invisible=False, zero_area=False):
    rng = np.random.default_rng(seed)
    W, H = clip
    B = len(counts)
    nkpt, ndim = kpt_shape
    spread = 1.4 * float(np.mean(sigma_of(kpt_shape)))  # a displacement of spread * sqrt(w h) per axis brings OKS to about 0.45
    rows = (rng.standard_normal((B, max_det, 6)) * 1e3).astype(np.float32)  # garbage beyond the counts
    kpts = (rng.standard_normal((B, max_det, nkpt, ndim)) * 1e3).astype(np.float32)
    tbox, tkpt, tcls, timg = [], [], [], []
    for i, (cnt, nl) in enumerate(zip(counts, nlab)):
        cx, cy = rng.uniform(0.15 * W, 0.85 * W, nl), rng.uniform(0.15 * H, 0.85 * H, nl)
        bw, bh = rng.uniform(0.06 * W, 0.2 * W, nl), rng.uniform(0.1 * H, 0.3 * H, nl)
        if outside and nl >= 4:
            cx[0], cy[1] = 0.01 * W, 0.99 * H   # boxes cut by the left and the bottom edge: keypoints outside the image
            cx[2], cy[3] = 0.98 * W, 0.02 * H
        if zero_area and nl >= 2:
            cx[0], bw[0] = W + 40.0, 30.0       # wholly right of the image: x1 and x2 both clip to W
        lb = np.stack((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), 1)
        lk = np.concatenate((np.stack((cx[:, None] + (rng.random((nl, nkpt)) - 0.5) * bw[:, None], cy[:, None] + (rng.random((nl, nkpt)) - 0.5) * bh[:, None]), 2),
                             rng.integers(0, 3, (nl, nkpt, 1)).astype(np.float64)), 2)
        none = lk[..., 2].sum(1) == 0
        lk[none, 0, 2] = 2.0  # at least one visible keypoint per label ...
        if invisible and i == 0 and nl >= 3:
            lk[0, :, 2] = 0.0                      # ... except here: no visible keypoint (the reference's 0 / eps)
            lk[1, :, 2], lk[1, nkpt // 2, 2] = 0.0, 1.0  # a single visible keypoint
        lc = rng.integers(0, NC, nl).astype(np.float32)
        if cnt:
            if nl:
                src = rng.integers(0, nl, cnt)
                src[: min(cnt, nl)] = np.arange(min(cnt, nl))  # every label has a detection of its own
                u = rng.random(cnt) ** 2
                scale = spread * np.sqrt(bw[src] * bh[src])
                pk = lk[src][..., :2] + rng.normal(0, 1, (cnt, nkpt, 2)) * (u * scale)[:, None, None]
                pc = lc[src].copy()
                flip = rng.random(cnt) < 0.15
                pc[flip] = (pc[flip] + rng.integers(1, NC, int(flip.sum()))) % NC
                order = rng.permutation(cnt)
                pk, pc = pk[order], pc[order]
            else:
                pk = np.stack((rng.uniform(0, W, (cnt, nkpt)), rng.uniform(0, H, (cnt, nkpt))), 2)
                pc = rng.integers(0, NC, cnt).astype(np.float32)
            if outside:
                pk[: cnt // 3] += rng.normal(0, 1, (cnt // 3, 1, 2)) * 0.02 * W  # whole skeletons pushed about, some over the edges
            kpts[i, :cnt, :, :2] = pk
            if ndim == 3:
                kpts[i, :cnt, :, 2] = rng.random((cnt, nkpt))  # the predictions' visibility: not used by the score
            rows[i, :cnt, :4] = rng.uniform(0, W, (cnt, 4))
            rows[i, :cnt, 4] = np.sort(rng.uniform(0.001, 1, cnt))[::-1]
            rows[i, :cnt, 5] = pc
        tbox.append(lb), tkpt.append(lk), tcls.append(lc), timg.append(np.full(nl, i))
    tbox = np.concatenate(tbox).astype(np.float32)
    lim = np.array([W, H, W, H], np.float32)
    tbox = np.minimum(np.maximum(tbox, 0), lim)  # what _prepare_batch leaves
    tkpt = clip_kpts(np.concatenate(tkpt).astype(np.float32), W, H)
    tcls, timg = np.concatenate(tcls), np.concatenate(timg).astype(np.int32)
    perm = rng.permutation(len(tbox))  # batch layout: labels belong to images by value, in no order
    return dict(rows=rows, kpts=kpts, counts=np.array(counts, np.int32), tbox=tbox[perm], tkpt=tkpt[perm], tcls=tcls[perm], timg=timg[perm], clip=(W, H),
                max_det=max_det, single_cls=False, kpt_shape=tuple(kpt_shape))


def _rank_case():
    """Two detections whose best label is the same one; the higher-ranked detection has the LOWER OKS (about 0.72 against 0.93)."""
    rng = np.random.default_rng(5)
    lb = np.array([[60.0, 50.0, 140.0, 210.0], [200.0, 40.0, 270.0, 200.0]], np.float32)
    lk = np.zeros((2, 17, 3), np.float32)
    for j in range(2):
        lk[j, :, 0] = rng.uniform(lb[j, 0], lb[j, 2], 17)
        lk[j, :, 1] = rng.uniform(lb[j, 1], lb[j, 3], 17)
    lk[..., 2] = 2.0
    rows = np.full((1, 4, 6), 9e5, np.float32)
    kpts = np.full((1, 4, 17, 3), 9e5, np.float32)
    kpts[0, 0, :, :2] = lk[0, :, :2] + np.float32(3.7)
    kpts[0, 1, :, :2] = lk[0, :, :2] + np.float32(1.6)
    kpts[0, :2, :, 2] = 0.9
    rows[0, 0, 4:], rows[0, 1, 4:] = (0.9, 1.0), (0.8, 1.0)
    return dict(rows=rows, kpts=kpts, counts=np.array([2], np.int32), tbox=lb, tkpt=lk, tcls=np.array([1.0, 1.0], np.float32), timg=np.zeros(2, np.int32),
                clip=(320, 256), max_det=4, single_cls=False, kpt_shape=(17, 3))


def match_inputs(name, seed):
    if name == "rank":
        return _rank_case()
    if name == "single_cls":
        c = _gen(seed, **MATCH_CASES[SINGLE_CLS_OF])
        c["tcls"] = np.zeros_like(c["tcls"])  # (what single_cls makes of a dataset: every label is class 0)
        c["single_cls"] = True
        return c
    return _gen(seed, **MATCH_CASES[name])


def bound_case():
    """The LDS layout at its upper bound: max_det 4096, all rows kept, 32 keypoints (the cap; the generic instance), 5 labels of 40 x 40 px
    200 px apart.  The first five detections are copies of the labels, the rest skeletons far away of a class no label has.  No seed: every
    same-class pair scores 1 or below 1e-6."""
    rng = np.random.default_rng(0)
    nkpt = 32
    c0 = np.array([[100.0, 100.0], [300.0, 100.0], [500.0, 100.0], [100.0, 300.0], [300.0, 300.0]])
    lb = np.concatenate((c0 - 20, c0 + 20), 1).astype(np.float32)
    lk = np.concatenate((c0[:, None] + rng.uniform(-20, 20, (5, nkpt, 2)), np.full((5, nkpt, 1), 2.0)), 2).astype(np.float32)
    rows = np.zeros((1, 4096, 6), np.float32)
    kpts = rng.uniform(600, 1000, (1, 4096, nkpt, 2)).astype(np.float32)
    rows[0, :, 4], rows[0, :, 5] = np.linspace(0.99, 0.01, 4096), 2.0
    kpts[0, :5], rows[0, :5, 5] = lk[..., :2], (0.0, 1.0, 0.0, 1.0, 0.0)
    return dict(rows=rows, kpts=kpts, counts=np.array([4096], np.int32), tbox=lb, tkpt=lk, tcls=np.array([0.0, 1.0, 0.0, 1.0, 0.0], np.float32),
                timg=np.zeros(5, np.int32), clip=(1100, 1040), max_det=4096, single_cls=False, kpt_shape=(nkpt, 2))


def full_stage_case():
    """A stage filled exactly to capacity: STAGE + 1 labels of one class, all of image 0 and in order (the first step stages STAGE entries, the
    second one); detections = exact copies of labels 0, STAGE - 1 and STAGE, and a second copy of label STAGE ranked below the first.  30 x 30 px
    boxes 60 px apart: every same-class pair scores 1 or below 1e-6."""
    rng = np.random.default_rng(1)
    n = STAGE + 1
    i = np.arange(n)
    c0 = np.stack((40.0 + 60.0 * (i % 9), 40.0 + 60.0 * (i // 9)), 1)
    lb = np.concatenate((c0 - 15, c0 + 15), 1).astype(np.float32)
    lk = np.concatenate((c0[:, None] + rng.uniform(-15, 15, (n, 17, 2)), np.full((n, 17, 1), 1.0)), 2).astype(np.float32)
    rows = np.zeros((1, 4, 6), np.float32)
    kpts = np.zeros((1, 4, 17, 3), np.float32)
    kpts[0, :, :, :2] = lk[[0, STAGE - 1, STAGE, STAGE], :, :2]
    rows[0, :, 4], rows[0, :, 5] = (0.9, 0.8, 0.7, 0.6), 1.0
    return dict(rows=rows, kpts=kpts, counts=np.array([4], np.int32), tbox=lb, tkpt=lk, tcls=np.ones(n, np.float32), timg=np.zeros(n, np.int32), clip=(640, 560),
                max_det=4, single_cls=False, kpt_shape=(17, 3))


def expect64(c):
    """``rule64`` on a one-image case whose labels are in image order: tp (max_det, T), best_label (max_det,), and the float64 scores of the
    same-class pairs."""
    cnt = int(c["counts"][0])
    o = oks64(c["tbox"], c["tkpt"], clip_kpts(c["kpts"][0, :cnt], *c["clip"]), sigma_of(c["kpt_shape"]))
    same = c["tcls"][:, None] == c["rows"][0, :cnt, 5][None]
    tp, best, _ = rule64(np.where(same, o, 0.0))
    full_tp, full_best = np.zeros((c["max_det"], len(IOUV)), bool), np.full(c["max_det"], -1, np.int64)
    full_tp[:cnt], full_best[:cnt] = tp, best
    return full_tp, full_best, o[same]


def dense_form(c, nc=NC, anchors=96, seed=0):
    """The case's predictions as the head hands them on: pred (B, 4 + nc + nk, A) with the kept rows' keypoints at distinct random anchors and
    noise elsewhere, and the NMS's index (B, max_det) whose entries beyond the counts are poison."""
    rng = np.random.default_rng(seed)
    B, md = len(c["counts"]), c["max_det"]
    nkpt, ndim = c["kpt_shape"]
    A = max(anchors, md + 7)
    pred = (rng.standard_normal((B, 4 + nc + nkpt * ndim, A)) * 50).astype(np.float32)
    index = np.full((B, md), 0x7FFFFFF0, np.int32)
    index[:, 1::2] = -12345
    for b, cnt in enumerate(c["counts"]):
        a = rng.permutation(A)[:cnt]
        index[b, :cnt] = a
        pred[b, 4 + nc :, a] = c["kpts"][b, :cnt].reshape(cnt, nkpt * ndim)
    return pred, index


def match_evaluate(c, oks32, match32, kpts64=None, floor=0.0, fixed=None):
    """Evaluates a case in float64 and in fp32 (``oks32(tbox (L, 4), tkpt (L, nkpt, 3), pred (D, nkpt, ndim) clipped, sigma) -> (L, D)`` fp32
    array, ``match32(pred_cls, true_cls, oks) -> (D, T)`` bool: the reference's functions in the builder, this package's restatements in the
    tests).  Returns M, the float64 tp / best_iou / best_label (batch layout, label positions in tbox), the fp32 tp, the fp32 scores per image
    and ``ok``: the acceptance conditions.  ``kpts64``: the float64 side's own predictions (the rows of a float64 model run) instead of
    ``c["kpts"]``.  ``floor``: the M of the ``val300`` case (300 detections x 40 labels, the validator's load): a case of a handful of pairs
    does not sample the fp32 error of the expression, so its margin is never taken below that one -- a larger margin makes the acceptance
    conditions stricter.  ``fixed``: the M to judge the conditions with (the tests: the recorded margin; fp32 exp of another CPU differs in the
    last bit; ``M_meas`` is what this call measured)."""
    B, md = len(c["counts"]), c["max_det"]
    W, H = c["clip"]
    sigma = sigma_of(c["kpt_shape"])
    tp64, tp32 = np.zeros((B, md, len(IOUV)), bool), np.zeros((B, md, len(IOUV)), bool)
    biou64, best64 = np.zeros((B, md)), np.full((B, md), -1, np.int64)
    worst, per_image = 0.0, []
    for i, cnt in enumerate(c["counts"]):
        where = np.nonzero(c["timg"] == i)[0]
        if cnt == 0 or len(where) == 0:
            continue
        det = clip_kpts(c["kpts"][i, :cnt], W, H)
        det64 = det if kpts64 is None else clip_kpts(np.asarray(kpts64[i, :cnt], np.float64), W, H)
        pcls = np.zeros(cnt, np.float32) if c["single_cls"] else c["rows"][i, :cnt, 5]
        lab, lk, lcls = c["tbox"][where], c["tkpt"][where], c["tcls"][where]
        o64 = oks64(lab, lk, det64, sigma)
        o32 = np.asarray(oks32(lab, lk, det, sigma), np.float32)
        same = lcls[:, None] == pcls[None]
        per_image.append((o64, o32.astype(np.float64), same))
        band = same & (o64 >= BAND_LO)
        if band.any():
            worst = max(worst, float(np.abs(o32 - o64)[band].max()))
        t, b, v = rule64(np.where(same, o64, 0.0))
        tp64[i, :cnt], biou64[i, :cnt], best64[i, :cnt] = t, v, np.where(b >= 0, where[np.maximum(b, 0)], -1)
        tp32[i, :cnt] = match32(pcls, lcls, o32)
    M = max(8 * worst, floor) if fixed is None else fixed
    ok, near = True, np.inf
    for o64, o32, same in per_image:
        ok &= not np.isnan(o64).any() and not np.isnan(o32).any()
        v = np.where(same, o64, -1.0)
        dist = np.abs(v[:, :, None] - IOUV[None, None])
        ok &= not (dist <= M)[v >= 0].any()  # no pair within the margin of a threshold
        near = min(near, float(dist[v >= 0].min(initial=np.inf)))
        if v.shape[0] > 1:
            top2 = np.sort(v, 0)[-2:]
            ok &= not ((top2[1] >= 0.5 - M) & (top2[1] - top2[0] <= M)).any()  # the two best same-class labels of a detection that can reach 0.5 are apart
    ok &= bool(np.array_equal(tp64, tp32))
    return dict(M=M, tp64=tp64, tp32=tp32, best_iou64=biou64, best_label64=best64, ok=bool(ok), near=near, M_meas=8 * worst, oks32=[p[1] for p in per_image])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
E2E = {  # tag -> (yaml, images, batch)
    "pv3": ("yolov8-pose.yaml", 4, 3),
    "pvp2": ("yolov8-p2-repvgg-pose.yaml", 3, 2),
}
E2E_HW, E2E_NC = (64, 96), 2


def e2e_images(seed, n):
    return torch.randint(0, 256, (n, 3, *E2E_HW), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
