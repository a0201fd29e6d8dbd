"""Cases, a float64 restatement and the checks of the mask term of the segmentation loss (``dy_seg_loss``), shared by
tests/test_seg_loss_host.py (CPU) and tests/test_seg_loss_gpu.py, in the style of tests/_loss_util.py.  Plain CPU torch; not collected.

The restatement (``seg_from_owner64``) follows calculate_segmentation_loss / single_mask_loss / crop_mask of the reference's
v8SegmentationLoss (overlap_mask=True) in float64 on the SAME fp32 label table, coefficient maps, prototypes and index maps the device
gets, as a function of an owner map (anchor -> label row, -1 = background): the foreground set is ``owner >= 0``.  The crop is NOT computed
in float64: whether prototype column r lies in a label's crop is the fp32 comparison ``r >= (x1 / W) * mw`` of the reference, in the
reference's order of operations.  ``kernel_crop32`` restates what csrc/seg_loss.hip computes instead (the same fp32 products, then
ceil / clamp to an integer range) and tests/test_seg_loss_host.py requires it to equal the real reference's stored crop masks pixel for
pixel on every case: the unsure set is empty by condition.

Every case compared with the real reference (tests/golden/seg_loss.npz, written by tools/make_seg_loss_golden.py) has the reference's
``fg_mask`` equal to ``target_scores.sum(-1) > 0`` at every anchor, and an empty unsure set of tests/_loss_util.py::assign64, so the device's
owner map must equal the reference's; head seeds (_SEEDS) are chosen for that (the golden tool asserts both and prints the seeds to use).

``thin`` is the one case without a reference run.  A label that owns an anchor contains that anchor's centre, and the centres of every
stride (s/2 + k s) fall on whole prototype columns, so under a real assignment a crop is never empty; the kernel's empty-crop path (term 0,
the anchor still counted in n_fg) is therefore driven with a hand-made owner map and compared with the restatement alone.

Bars: per case 16 x the real fp32 reference's own error against its float64 run (``ref_err`` in the golden: items relative with the floor
ITEM_FLOOR, gradients relative to the map's largest entry), floored at 16 fp32 ulps, capped at the detection loss's 2e-4 / 1e-4.
Measured on an MI355X (tests/test_seg_loss_gpu.py prints them): see MEASURED below.
"""
from __future__ import annotations

from functools import lru_cache
from pathlib import Path

import numpy as np
import torch

from tests import _loss_util as LU

GOLDEN = Path(__file__).parent / "golden" / "seg_loss.npz"
NM = 32
GAINS = LU.GAINS  # box (also the mask term's), cls, dfl
L3, L4 = (8.0, 16.0, 32.0), (4.0, 8.0, 16.0, 32.0)
MUTANTS = ("x1_gt", "x2_le", "mean_crop", "area_px", "label_count", "mask_k", "swap_hw", "ratio2_roundup", "class_gain", "no_batch")
# largest errors of dy_seg_loss against the restatement over all cases, measured on an MI355X: (items, gradients); the bars they met
MEASURED = dict(items=7.4e-8, grad=2.8e-7)  # cases pad and edge0-C4; bars 1.9e-6 .. 1.0e-5 and 1.9e-6 .. 5.8e-6


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def _paint(gt, hw, ghw, order=None):
    """Overlap index maps (B, gh, gw) int64 from a label table: per image every valid row's box-inscribed ellipse, painted in descending-area
    order (or ``order[b]``, a list of rows) with the ROW's index + 1, so a later (smaller) label wins where two overlap."""
    B, G = gt.shape[:2]
    H, W = hw
    gh, gw = ghw
    out = torch.zeros(B, gh, gw, dtype=torch.int64)
    ys, xs = (torch.arange(gh, dtype=torch.float64) + 0.5) * (H / gh), (torch.arange(gw, dtype=torch.float64) + 0.5) * (W / gw)
    for b in range(B):
        box = gt[b, :, 1:5].double()
        rows = [g for g in range(G) if float(box[g].sum()) > 0]
        area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
        rows = order[b] if order is not None and order[b] is not None else sorted(rows, key=lambda g: (-float(area[g]), g))
        for g in rows:
            cx, cy, rx, ry = (box[g, 0] + box[g, 2]) / 2, (box[g, 1] + box[g, 3]) / 2, (box[g, 2] - box[g, 0]) / 2, (box[g, 3] - box[g, 1]) / 2
            inside = ((xs[None] - cx) / rx) ** 2 + ((ys[:, None] - cy) / ry) ** 2 <= 1.0
            out[b][inside] = g + 1
    return out


def _edge_rows(step, half=False):
    """Boxes whose edges are multiples of 4 px (whole prototype columns on both grids); step +1 / -1: every edge one fp32 ulp inward /
    outward; ``half``: edges at 4 k + 2 (half-integer columns on the 16-wide grid, whole ones on the 32-wide)."""
    base = [[1, 8.0, 12.0, 40.0, 36.0], [4, 12.0, 20.0, 44.0, 52.0], [7, 4.0, 24.0, 56.0, 40.0], [9, 16.0, 16.0, 48.0, 48.0]]
    if half:
        return [[c, x1 + 2, y1 + 2, x2 - 2, y2 - 2] for c, x1, y1, x2, y2 in base]
    if step == 0:
        return base
    return [[c, LU._ulp(x1, step), LU._ulp(y1, step), LU._ulp(x2, -step), LU._ulp(y2, -step)] for c, x1, y1, x2, y2 in base]


def _crowd_rows(seed, n=10):
    g = torch.Generator().manual_seed(seed)
    j = torch.rand(n, 4, generator=g) * 6
    return [[i % 10, 14.0 + float(j[i, 0]), 14.0 + float(j[i, 1]), 44.0 + float(j[i, 2]), 44.0 + float(j[i, 3])] for i in range(n)]


_SEEDS: dict = {'rand-R3': 2, 'rect-C4': 1, 'ld40-C4': 1}  # per case id, where another head seed than the default was needed (tools/make_seg_loss_golden.py --seeds)
# id -> (levels, (H, W), kind, options)
_SPECS = {
    "conv-C3": (L3, (64, 64), "C", {}), "conv-C4": (L4, (64, 64), "C", {}),
    "rand-R3": (L3, (64, 64), "R", {}), "rand-R4": (L4, (64, 64), "R", {}),
    "edge0-C3": (L3, (64, 64), "C", dict(rows=lambda: [_edge_rows(0), _edge_rows(0)[::-1]])),
    "edge0-C4": (L4, (64, 64), "C", dict(rows=lambda: [_edge_rows(0), _edge_rows(0)[::-1]])),
    "edgeP-C3": (L3, (64, 64), "C", dict(rows=lambda: [_edge_rows(1), _edge_rows(1)[::-1]])),
    "edgeM-C3": (L3, (64, 64), "C", dict(rows=lambda: [_edge_rows(-1), _edge_rows(-1)[::-1]])),
    "edgeH-C3": (L3, (64, 64), "C", dict(rows=lambda: [_edge_rows(0, True), _edge_rows(0, True)[::-1]])),
    # image 0: rows 0 and 1 overlap; row 2 lies inside row 0 and is painted FIRST, so nothing of it is left in the map
    "overlap": (L3, (64, 64), "C", dict(rows=lambda: [[[0, 8.0, 8.0, 40.0, 40.0], [1, 24.0, 24.0, 56.0, 56.0], [2, 14.0, 14.0, 30.0, 30.0]],
                                                       [[3, 4.0, 20.0, 36.0, 60.0], [5, 20.0, 4.0, 60.0, 44.0]]], order=[[2, 0, 1], None])),
    "whole": (L3, (64, 64), "C", dict(rows=lambda: [[[3, 0.0, 0.0, 64.0, 64.0], [1, 20.0, 20.0, 44.0, 40.0]], [[6, 0.0, 0.0, 64.0, 64.0]]])),
    "crowd": (L3, (64, 64), "C", dict(rows=lambda: [_crowd_rows(7), _crowd_rows(8, 9)])),
    "pad": (L3, (64, 64), "C", dict(rows=lambda: [[LU._rand_boxes(31, 1, 10, (64, 64))[0], None, LU._rand_boxes(32, 1, 10, (64, 64))[0], None, LU._rand_boxes(33, 1, 10, (64, 64))[0]],
                                                   [None, LU._rand_boxes(34, 1, 10, (64, 64))[0], None, LU._rand_boxes(35, 1, 10, (64, 64))[0]]])),
    "none": (L3, (64, 64), "R", dict(rows=lambda: [[], []])),
    "half": (L3, (64, 64), "C", dict(rows=lambda: [LU._rand_boxes(41, 4, 10, (64, 64)), []])),
    "sat": (L3, (64, 64), "C", dict(scale=3.3)),
    "rect-C3": (L3, (64, 96), "C", {}), "rect-C4": (L4, (64, 96), "C", {}),
    "ld36-C3": (L3, (64, 64), "C", dict(ld=36)), "ld40-C4": (L4, (64, 64), "C", dict(ld=40)),
    "i32-C3": (L3, (64, 64), "C", dict(mask_dtype=torch.int32)),
    "bf16-C3": (L3, (64, 64), "C", dict(proto_dtype=torch.bfloat16)),
}
CASE_IDS = list(_SPECS)  # the cases with a reference run
VARIANT_IDS = ("ld36-C3", "ld40-C4", "i32-C3")  # device-side layout variants of the conv cases: the golden keeps no gradients for them (its size)
ALL_IDS = CASE_IDS + ["thin"]


def _seed(cid):
    return _SEEDS.get(cid, 100 + sum(map(ord, cid)))


def _finish(cid, feats, gt, strides, hw, opt, owner=None):
    B = gt.shape[0]
    seed = _seed(cid)
    g = torch.Generator().manual_seed(seed + 77)
    scale = opt.get("scale", 1.0)
    coefs = [torch.randn(B, NM, int(hw[0] // s), int(hw[1] // s), generator=g) * 0.5 * scale for s in strides]
    mhw = (int(hw[0] // strides[0]) * 2, int(hw[1] // strides[0]) * 2)  # Proto upsamples the first level 2 x
    proto = torch.randn(B, NM, *mhw, generator=g) * 0.5 * scale
    pd = opt.get("proto_dtype", torch.float32)
    proto = proto.to(pd).float()  # the values the device reads, as fp32 for the reference
    ghw = (hw[0] // 4, hw[1] // 4)
    masks = _paint(gt, hw, ghw, opt.get("order"))
    return dict(id=cid, feats=feats, coefs=coefs, proto=proto, proto_dtype=pd, masks=masks.to(opt.get("mask_dtype", torch.uint8)), gt=gt, strides=list(strides),
                nc=10, topk=10, hw=hw, ld=opt.get("ld", NM), owner=owner)


def build_case(cid):
    if cid == "thin":
        # label 0 is narrower than one prototype pixel (2 px on the 32-wide grid) and holds no whole column: x1m = 4.6, x2m = 4.95
        gt = LU._table([[[2, 9.2, 8.0, 9.9, 40.0], [5, 20.0, 20.0, 52.0, 44.0]], [[1, 30.0, 1.1, 50.0, 1.9]]])
        feats = LU._rand_heads(5, 2, 10, (64, 64), L4)
        A = sum(f.shape[2] * f.shape[3] for f in feats)
        owner = torch.full((2, A), -1, dtype=torch.int64)
        owner[0, 34], owner[0, 300], owner[0, 301], owner[0, 256 + 40], owner[1, 7] = 0, 1, 1, 0, 0
        return _finish(cid, feats, gt, L4, (64, 64), {}, owner=owner)
    strides, hw, kind, opt = _SPECS[cid]
    seed = _seed(cid)
    if "rows" in opt:
        gt = LU._table(opt["rows"]())
    else:
        gt = LU._table([LU._rand_boxes(seed * 3 + b, 4, 10, hw) for b in range(2)])
    feats = LU._rand_heads(seed, 2, 10, hw, strides) if kind == "R" else LU._converged_heads(seed, gt, 10, hw, strides)
    return _finish(cid, feats, gt, strides, hw, opt)


def train_labels(seed, hw=(64, 96), nc=10):
    """Labels and index maps of the training fixtures (tests/golden/seg_train.npz): 4 + 3 boxes of 0.1 .. 0.6 of the image, per image sorted by
    area (largest first), the maps at a quarter of the image painted in that order (``_paint``): value k + 1 = the image's k-th label."""
    H, W = hw
    per = []
    for b, n in enumerate((4, 3)):
        rows = LU._rand_boxes(seed + b, n, nc, hw)
        per.append(sorted(rows, key=lambda r: -(r[3] - r[1]) * (r[4] - r[2])))
    masks = _paint(LU._table(per), hw, (H // 4, W // 4)).to(torch.uint8)
    bi = torch.cat([torch.full((len(r),), float(b)) for b, r in enumerate(per)])
    rows = torch.tensor([r for p in per for r in p], dtype=torch.float32)
    xywh = torch.stack(((rows[:, 1] + rows[:, 3]) / 2 / W, (rows[:, 2] + rows[:, 4]) / 2 / H, (rows[:, 3] - rows[:, 1]) / W, (rows[:, 4] - rows[:, 2]) / H), 1)
    return {"batch_idx": bi, "cls": rows[:, :1].clone(), "bboxes": xywh, "masks": masks}


# ---- the crop: fp32, in the reference's order of operations -----------------------------------------------------------------------
def _mxyxy32(box, hw, mhw, swap_hw=False):
    """(n, 4) fp32 pixel boxes -> the fp32 box on the prototype grid: (x / W) * mw, divide then multiply (loss.py:417-423)."""
    H, W = (hw[1], hw[0]) if swap_hw else hw
    norm = box.float() / torch.tensor([W, H, W, H], dtype=torch.float32)
    return norm, norm * torch.tensor([mhw[1], mhw[0], mhw[1], mhw[0]], dtype=torch.float32)


def kernel_crop32(box, hw, mhw):
    """What csrc/seg_loss.hip computes: per box the integer ranges [c0, c1) x [r0, r1) = clamp(ceil(.), 0, size) of the fp32 grid box, as a
    (n, mh, mw) bool mask."""
    _, m = _mxyxy32(box, hw, mhw)
    mh, mw = mhw
    c0, c1 = m[:, 0].ceil().clamp(0, mw).long(), m[:, 2].ceil().clamp(0, mw).long()
    r0, r1 = m[:, 1].ceil().clamp(0, mh).long(), m[:, 3].ceil().clamp(0, mh).long()
    r, c = torch.arange(mw)[None, None, :], torch.arange(mh)[None, :, None]
    return (r >= c0[:, None, None]) & (r < c1[:, None, None]) & (c >= r0[:, None, None]) & (c < r1[:, None, None])


def reference_crop32(box, hw, mhw, mut=()):
    """crop_mask's comparisons (utils/ops.py:660-676) on the fp32 grid box."""
    _, m = _mxyxy32(box, hw, mhw, swap_hw="swap_hw" in mut)
    x1, y1, x2, y2 = (m[:, i, None, None] for i in range(4))
    r, c = torch.arange(mhw[1], dtype=torch.float32)[None, None, :], torch.arange(mhw[0], dtype=torch.float32)[None, :, None]
    left = (r > x1) if "x1_gt" in mut else (r >= x1)
    right = (r <= x2) if "x2_le" in mut else (r < x2)
    return left & right & (c >= y1) & (c < y2)


def positives(owner):
    """[(image, anchor, label row)] in the kernel's order: by image, then anchor."""
    return [(int(b), int(a), int(owner[b, a])) for b, a in (owner >= 0).nonzero().tolist()]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def seg_from_owner64(case, owner, mut=(), want_grad=True):
    """(seg, seg's contribution to the total, [d contribution / d coef level], d contribution / d proto) in float64."""
    B = case["gt"].shape[0]
    hw = case["hw"]
    coefs = [c.double().requires_grad_(want_grad) for c in case["coefs"]]
    proto = case["proto"].double().requires_grad_(want_grad)
    mh, mw = proto.shape[2:]
    masks = case["masks"].long()
    if tuple(masks.shape[1:]) != (mh, mw):  # F.interpolate(nearest) at scale 2: prototype pixel (y, x) reads map pixel (y >> 1, x >> 1)
        iy, ix = torch.arange(mh) >> 1, torch.arange(mw) >> 1
        if "ratio2_roundup" in mut:
            iy, ix = ((torch.arange(mh) + 1) >> 1).clamp(max=masks.shape[1] - 1), ((torch.arange(mw) + 1) >> 1).clamp(max=masks.shape[2] - 1)
        masks = masks[:, iy][:, :, ix]
    pm = torch.cat([c.reshape(B, NM, -1) for c in coefs], 2).permute(0, 2, 1)  # (B, A, 32)
    owner = owner.long()
    total = torch.zeros((), dtype=torch.float64)
    for b in range(B):
        idx = (owner[b] >= 0).nonzero().flatten()
        if idx.numel() == 0:
            continue
        g = owner[b, idx]
        box = case["gt"][b, g, 1:5]
        norm, _ = _mxyxy32(box, hw, (mh, mw), swap_hw="swap_hw" in mut)
        crop = reference_crop32(box, hw, (mh, mw), mut).double()
        z = (pm[b, idx] @ proto[b].reshape(NM, -1)).reshape(-1, mh, mw)
        t = (masks[b][None] == (g if "mask_k" in mut else g + 1)[:, None, None]).double()
        l = z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
        n64 = norm.double()
        area = (n64[:, 2] - n64[:, 0]) * (n64[:, 3] - n64[:, 1])
        if "area_px" in mut:
            area = area * (hw[0] * hw[1])
        s = (l * crop).sum((1, 2))
        per = s / crop.sum((1, 2)).clamp(min=1) if "mean_crop" in mut else s / (mh * mw)
        total = total + (per / area).sum()
    nfg = int((owner >= 0).sum())
    div = int((case["gt"][..., 1:5].sum(-1) > 0).sum()) if "label_count" in mut else nfg
    gain = GAINS[1] if "class_gain" in mut else GAINS[0]
    seg = gain * total / div if nfg > 0 and div > 0 else total * 0.0
    contrib = seg * (1 if "no_batch" in mut else B)
    if not want_grad:
        return seg.detach(), contrib.detach(), None, None
    if nfg == 0:
        return seg.detach(), contrib.detach(), [torch.zeros_like(c) for c in coefs], torch.zeros_like(proto)
    grads = torch.autograd.grad(contrib, [*coefs, proto], allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(x) for g, x in zip(grads, [*coefs, proto])]
    return seg.detach(), contrib.detach(), list(grads[:-1]), grads[-1]


# ---- goldens, bars, checks -------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _golden_file():
    return dict(np.load(GOLDEN))


def golden(cid):
    pre = cid + "/"
    return {k[len(pre):]: v for k, v in _golden_file().items() if k.startswith(pre)}


def bars(cid):
    """(items bar, gradient bar) of a case: 16 x the real fp32 reference's own error (floored at fp32's rounding), capped at the ceilings."""
    if cid == "thin":
        e_items = e_grad = 0.0  # no reference run: the floor alone
    else:
        e_items, e_grad = (float(v) for v in golden(cid)["ref_err"])
    return min(LU.ITEM_CEIL, LU.FACTOR * max(e_items, LU.F32_EPS)), min(LU.GRAD_CEIL, LU.FACTOR * max(e_grad, LU.F32_EPS))


@lru_cache(maxsize=None)
def case_reference(cid):
    """(case, owner map, float64 result under it): computed once per case and shared; callers leave it unchanged."""
    case = build_case(cid)
    owner = case["owner"] if case["owner"] is not None else torch.from_numpy(golden(cid)["owner"]).long()
    return case, owner, seg_from_owner64(case, owner)


def check_result(cid, out, gcoef, gproto, ref=None):
    """Errors of (out[2] = seg, contribution; gradient maps or None) against the float64 restatement, and the bars: a dict with ``ok``."""
    _, _, r = case_reference(cid)
    seg, contrib, rc, rp = r if ref is None else ref
    out = torch.as_tensor(out).detach().cpu().double().flatten()
    e_items = LU.item_err(out, torch.stack((seg, contrib))) if bool(torch.isfinite(out).all()) else float("inf")
    e_grad = LU.grad_err([*gcoef, gproto], [*rc, rp]) if gproto is not None else 0.0
    bi, bg = bars(cid)
    return dict(items_err=e_items, items_bar=bi, grad_err=e_grad, grad_bar=bg, ok=e_items <= bi and e_grad <= bg)
