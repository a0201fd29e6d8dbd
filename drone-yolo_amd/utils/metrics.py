"""Detection and segmentation metrics of the validation step (reference: ultralytics/utils/metrics.py ``box_iou`` :52-71, ``mask_iou`` :137-153, ``SegmentMetrics`` :899-1030, ``smooth`` :447-452,
``compute_ap`` :505-534, ``ap_per_class`` :537-623, ``Metric`` :626-760; ``BaseValidator.match_predictions``, engine/validator.py:224-264).

Host logic in numpy, as in the reference (its metrics leave the device too: validator.get_stats() does ``.cpu().numpy()``): a few
thousand kept rows per validation set.  ``box_iou`` and ``match_predictions`` are what the validator runs with ``device_match=False``
and what ``dy_val_match`` (csrc/val_match.hip, the default) is tested against; AP is computed here in both cases.  Every function restates the reference's arithmetic step by step and is pinned against the
reference's own functions on synthetic statistics (tests/golden/val_metrics.npz, oracle/make_golden.py::val_metric_vectors)."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz


def box_iou(box1: np.ndarray, box2: np.ndarray, eps: float = 1e-7) -> np.ndarray:
    """(N, 4) x (M, 4) xyxy -> (N, M) IoU in fp32 — metrics.py:52-71."""
    a = box1.astype(np.float32)[:, None, :]
    b = box2.astype(np.float32)[None, :, :]
    inter = np.clip(np.minimum(a[..., 2:], b[..., 2:]) - np.maximum(a[..., :2], b[..., :2]), 0, None).prod(2)
    return inter / ((a[..., 2:] - a[..., :2]).prod(2) + (b[..., 2:] - b[..., :2]).prod(2) - inter + np.float32(eps))


def mask_iou(mask1: np.ndarray, mask2: np.ndarray, eps: float = 1e-7) -> np.ndarray:
    """(N, n) x (M, n) flattened 0 / 1 masks -> (N, M) IoU in fp32 — metrics.py:137-153: the intersection as a float matrix product,
    ``(area1 + area2) - intersection`` and the division, each rounded to fp32 (all counts are integers below 2^24, so the sums are exact)."""
    a, b = mask1.astype(np.float32), mask2.astype(np.float32)
    inter = np.clip(a @ b.T, 0, None)
    union = (a.sum(1, dtype=np.float32)[:, None] + b.sum(1, dtype=np.float32)[None]) - inter
    return inter / (union + np.float32(eps))


def _covariance_terms(boxes):
    """(a, b, c) of the Gaussian of xywhr boxes (N, 5), each (N, 1) — metrics.py:178-195 (the centres play no part)."""
    a, b, r = boxes[:, 2:3].pow(2) / 12, boxes[:, 3:4].pow(2) / 12, boxes[:, 4:5]
    cos, sin = r.cos(), r.sin()
    cos2, sin2 = cos.pow(2), sin.pow(2)
    return a * cos2 + b * sin2, a * sin2 + b * cos2, (a - b) * cos * sin


def batch_probiou(obb1, obb2, eps: float = 1e-7):
    """(N, 5) x (M, 5) xywhr boxes (tensors or arrays) -> (N, M) ProbIoU tensor in the inputs' precision — metrics.py:244-275, in torch as
    there.  It is what ``dy_nms_rotated`` (csrc/obb.hip) evaluates pair by pair on the device and what that kernel is tested against."""
    import torch

    obb1 = torch.from_numpy(obb1) if isinstance(obb1, np.ndarray) else obb1
    obb2 = torch.from_numpy(obb2) if isinstance(obb2, np.ndarray) else obb2
    x1, y1 = obb1[:, 0:1], obb1[:, 1:2]
    x2, y2 = obb2[:, 0][None], obb2[:, 1][None]
    a1, b1, c1 = _covariance_terms(obb1)
    a2, b2, c2 = (t.squeeze(-1)[None] for t in _covariance_terms(obb2))
    det = (a1 + a2) * (b1 + b2) - (c1 + c2).pow(2)
    t1 = (((a1 + a2) * (y1 - y2).pow(2) + (b1 + b2) * (x1 - x2).pow(2)) / (det + eps)) * 0.25
    t2 = (((c1 + c2) * (x2 - x1) * (y1 - y2)) / (det + eps)) * 0.5
    t3 = (det / (4 * ((a1 * b1 - c1.pow(2)).clamp(min=0) * (a2 * b2 - c2.pow(2)).clamp(min=0)).sqrt() + eps) + eps).log() * 0.5
    bd = (t1 + t2 + t3).clamp(eps, 100.0)
    hd = (1.0 - (-bd).exp() + eps).sqrt()
    return 1 - hd


# the COCO keypoint constants (metrics.py:16-19): per-keypoint standard deviations, / 10
OKS_SIGMA = np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89]) / 10.0


def kpt_iou(kpt1, kpt2, area, sigma, eps: float = 1e-7):
    """(N, nkpt, 3) label keypoints x (M, nkpt, 2 | 3) predicted keypoints, (N,) label areas, nkpt sigmas -> (N, M) object keypoint
    similarity tensor in the inputs' precision — metrics.py:156-175, in torch, operation by operation as there (``sigma`` takes the keypoints'
    dtype; the mask count + eps is a default-dtype tensor).  It is what ``dy_val_oks_match`` (csrc/val_oks.hip) evaluates pair by pair on the
    device and what that kernel is tested against."""
    import torch

    kpt1 = torch.from_numpy(kpt1) if isinstance(kpt1, np.ndarray) else kpt1
    kpt2 = torch.from_numpy(kpt2) if isinstance(kpt2, np.ndarray) else kpt2
    area = torch.from_numpy(area) if isinstance(area, np.ndarray) else area
    d = (kpt1[:, None, :, 0] - kpt2[..., 0]).pow(2) + (kpt1[:, None, :, 1] - kpt2[..., 1]).pow(2)  # (N, M, nkpt)
    sigma = torch.tensor(np.asarray(sigma).tolist(), device=kpt1.device, dtype=kpt1.dtype)
    kpt_mask = kpt1[..., 2] != 0
    e = d / ((2 * sigma).pow(2) * (area[:, None, None] + eps) * 2)
    return ((-e).exp() * kpt_mask[:, None]).sum(-1) / (kpt_mask.sum(-1)[:, None] + eps)


def match_predictions(pred_classes: np.ndarray, true_classes: np.ndarray, iou: np.ndarray, iouv: np.ndarray) -> np.ndarray:
    """(D,) predicted classes, (L,) target classes, (L, D) IoU -> (D, len(iouv)) bool "correct" — validator.py:224-264 (the
    non-scipy branch: per threshold, matches sorted by IoU, each detection and then each label kept once)."""
    correct = np.zeros((pred_classes.shape[0], iouv.shape[0]), dtype=bool)
    correct_class = true_classes[:, None] == pred_classes
    iou = iou * correct_class
    for i, threshold in enumerate(iouv.tolist()):
        matches = np.array(np.nonzero(iou >= threshold)).T
        if matches.shape[0]:
            if matches.shape[0] > 1:
                matches = matches[iou[matches[:, 0], matches[:, 1]].argsort()[::-1]]
                matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
                matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
            correct[matches[:, 1].astype(int), i] = True
    return correct


def smooth(y: np.ndarray, f: float = 0.05) -> np.ndarray:
    """Box filter of fraction f — metrics.py:447-452."""
    nf = round(len(y) * f * 2) // 2 + 1
    p = np.ones(nf // 2)
    yp = np.concatenate((p * y[0], y, p * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def compute_ap(recall: np.ndarray, precision: np.ndarray) -> Tuple[float, np.ndarray, np.ndarray]:
    """101-point interpolated AP of one precision-recall curve — metrics.py:505-534."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    ap = _trapz(np.interp(x, mrec, mpre), x)
    return ap, mpre, mrec


def ap_per_class(tp: np.ndarray, conf: np.ndarray, pred_cls: np.ndarray, target_cls: np.ndarray, eps: float = 1e-16):
    """(tp, fp, p, r, f1, ap (nc, 10), unique_classes) — metrics.py:537-623 without the plots."""
    i = np.argsort(-conf)
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes, nt = np.unique(target_cls, return_counts=True)
    nc = unique_classes.shape[0]
    x = np.linspace(0, 1, 1000)
    ap, p_curve, r_curve = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l, n_p = nt[ci], i.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + eps)
        r_curve[ci] = np.interp(-x, -conf[i], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p_curve[ci] = np.interp(-x, -conf[i], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j], _, _ = compute_ap(recall[:, j], precision[:, j])
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    i = smooth(f1_curve.mean(0), 0.1).argmax()
    p, r, f1 = p_curve[:, i], r_curve[:, i], f1_curve[:, i]
    tp_n = (r * nt).round()
    fp_n = (tp_n / (p + eps) - tp_n).round()
    return tp_n, fp_n, p, r, f1, ap, unique_classes.astype(int)


class DetMetrics:
    """mean precision / recall / mAP50 / mAP50-95 and the fitness the trainer ranks checkpoints by — ``Metric`` (metrics.py:626-760:
    ``mean_results``, ``fitness`` with weights [0, 0, 0.1, 0.9]) behind ``DetMetrics.results_dict`` (:806-880)."""

    keys = ("metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)")

    def __init__(self):
        self.p = self.r = self.f1 = np.zeros(0)
        self.all_ap = np.zeros((0, 10))
        self.ap_class_index = np.zeros(0, dtype=int)

    def process(self, tp, conf, pred_cls, target_cls) -> None:
        res = ap_per_class(tp, conf, pred_cls, target_cls)
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = res[2], res[3], res[4], res[5], res[6]

    def mean_results(self):
        mp = self.p.mean() if len(self.p) else 0.0
        mr = self.r.mean() if len(self.r) else 0.0
        map50 = self.all_ap[:, 0].mean() if len(self.all_ap) else 0.0
        map_ = self.all_ap.mean() if len(self.all_ap) else 0.0
        return [mp, mr, map50, map_]

    @property
    def fitness(self) -> float:
        return float((np.array(self.mean_results()) * np.array([0.0, 0.0, 0.1, 0.9])).sum())

    @property
    def results_dict(self) -> Dict[str, float]:
        return dict(zip(self.keys + ("fitness",), [float(v) for v in self.mean_results()] + [self.fitness]))


class SegmentMetrics:
    """Box and mask metrics of a segmentation model — ``SegmentMetrics`` (metrics.py:899-1030): two ``Metric`` sets, fed by ``tp`` (boxes)
    and ``tp_m`` (masks) with the same ``conf`` / ``pred_cls`` / ``target_cls``; the same AP code as ``DetMetrics``.  ``fitness`` is the sum
    of the two sets' fitness."""

    keys = DetMetrics.keys + ("metrics/precision(M)", "metrics/recall(M)", "metrics/mAP50(M)", "metrics/mAP50-95(M)")

    def __init__(self):
        self.box, self.seg = DetMetrics(), DetMetrics()

    def process(self, tp, tp_m, conf, pred_cls, target_cls) -> None:
        self.seg.process(tp_m, conf, pred_cls, target_cls)
        self.box.process(tp, conf, pred_cls, target_cls)

    def mean_results(self):
        return self.box.mean_results() + self.seg.mean_results()

    @property
    def ap_class_index(self):
        return self.box.ap_class_index

    @property
    def fitness(self) -> float:
        return self.seg.fitness + self.box.fitness

    @property
    def results_dict(self) -> Dict[str, float]:
        return dict(zip(self.keys + ("fitness",), [float(v) for v in self.mean_results()] + [self.fitness]))


class OBBMetrics(DetMetrics):
    """Metrics of an oriented-box model — ``OBBMetrics`` (metrics.py): ``DetMetrics`` under its own name.  The statistics it is fed are
    matched on ProbIoU (``OBBValidator``); the AP code, the keys (the four (B) entries) and ``fitness`` are the detection ones."""


class PoseMetrics(SegmentMetrics):
    """Box and keypoint metrics of a pose model — ``PoseMetrics`` (metrics.py): ``SegmentMetrics``' shape with (P) keys: two ``Metric`` sets,
    fed by ``tp`` (boxes) and ``tp_p`` (keypoints: matched on OKS) with the same ``conf`` / ``pred_cls`` / ``target_cls``.  ``fitness`` is the sum
    of the two sets' fitness."""

    keys = DetMetrics.keys + ("metrics/precision(P)", "metrics/recall(P)", "metrics/mAP50(P)", "metrics/mAP50-95(P)")

    def __init__(self):
        self.box, self.pose = DetMetrics(), DetMetrics()

    def process(self, tp, tp_p, conf, pred_cls, target_cls) -> None:
        self.pose.process(tp_p, conf, pred_cls, target_cls)
        self.box.process(tp, conf, pred_cls, target_cls)

    def mean_results(self):
        return self.box.mean_results() + self.pose.mean_results()

    @property
    def fitness(self) -> float:
        return self.pose.fitness + self.box.fitness
