"""Cases, a dense float64 restatement and the checks of the oriented-box loss (``dy_obb_loss``), shared by tests/test_obb_loss_host.py
(CPU) and tests/test_obb_loss_gpu.py, in the style of tests/_loss_util.py.  Plain CPU torch; not collected.

The restatement follows v8OBBLoss (rotated TaskAlignedAssigner + BCE / ProbIoU / DFL) in float64 on the SAME fp32 label table, head maps
and angle-logit maps the device gets, in two halves:

* ``assign64_rot``: owner map, per-pair metric and overlap, ranked candidates, claim counts, with the kernel's documented deviation (a
  pick with metric exactly 0 is never taken) and tie rules (equal metrics: ascending anchor index; equal overlaps: first label index);
* ``loss_from_owner64_rot``: everything downstream as a function of an owner map alone, differentiable by float64 autograd (assignment and
  soft targets constant, nothing detached inside ProbIoU), so the numeric bars are evaluated under the DEVICE's owner map.  Metric and
  overlap of an owned pair are taken WITHOUT the in-box mask there: the owner map already says the device found the anchor inside.

Membership (is the anchor centre inside the rotated rectangle, edges included) is PINNED, not unsure: ``inbox32`` restates the reference's
four inequalities in fp32 in the reference's order of operations, which is what csrc/obb_loss.hip computes with contraction off, and
``case_reference`` hands that mask to ``assign64_rot``.  It equals the real reference's own mask on every case (test_obb_loss_host.py).  In
``edge`` it differs from the float64 inequalities at 11 pairs: the r = pi/2 labels put anchor centres on their edges, the fp32 value of
pi/2 moves those centres some 1e-8 of the edge's length off the edge in float64, and fp32 rounds that away again -- which is why the
float64 inequalities cannot decide the case the r = pi/2 labels were built for, and the fp32 ones are asked.

Unsure set: the only anchors whose owner may differ from ``assign64_rot``'s.  (a) rank-k / rank-(k+1) metric gaps below DELTA (non-zero);
(b) shared-anchor overlap gaps below DELTA (non-zero).  Exact ties and exact edge hits are pinned.  Without a membership mask (the mutants'
runs, the seed search) ``assign64_rot`` adds kind (c): anchors of which one of the four inequalities lies within DELTA, relative to the
edge's squared length, of equality in float64 without being exactly equal, and per label the anchors whose rank across the top-k boundary
depends on whether those count; label seeds are chosen so that (c) is empty too in every case but ``edge`` (27 anchors there, by construction).

DELTA = 16 * MEASURED_PAIR_ERR.  MEASURED_PAIR_ERR = 3.0e-5 is the largest relative difference between the real reference's fp32 metric or
overlap (tests/golden/obb_loss.npz, written by tools/make_obb_loss_golden.py) and this restatement's over all in-box pairs with a positive
metric of all cases (measured 2.95e-5, case thin; 2.2e-5 in conv, below 8e-6 elsewhere); test_obb_loss_host.py measures it again and
fails if a case exceeds it.  Label seeds (_LSEEDS) and head seeds (_SEEDS) are chosen so that the unsure set is EMPTY in every case.

Bars: per case 16 x the real reference's fp32 error against this restatement (under the reference's own owner map), floored at 16 fp32
ulps, capped at the detection loss's 2e-4 (items) and 1e-4 (gradients, relative to the map's largest entry).
"""
from __future__ import annotations

import math
from functools import lru_cache
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from tests import _loss_util as LU

MEASURED_PAIR_ERR = 3.0e-5
DELTA = 16 * MEASURED_PAIR_ERR
FACTOR, ITEM_CEIL, GRAD_CEIL, F32_EPS = LU.FACTOR, LU.ITEM_CEIL, LU.GRAD_CEIL, LU.F32_EPS
REG, GAINS, CLAMP = LU.REG, LU.GAINS, LU.CLAMP
HW = (64, 96)  # images are h != w
S3, S4 = (8.0, 16.0, 32.0), LU.S4
PI32 = float(torch.tensor(math.pi, dtype=torch.float32))
GOLDEN = Path(__file__).parent / "golden" / "obb_loss.npz"
MUTANTS = ("inbox_strict", "w_times_w", "dfl_rotated_target", "overlap_unclamped", "pixel_units_in_loss", "angle_centre_route_dropped", "mask_gt_on_xywh",
           "last_tie", "topk_minus_1")


# ---- label table: what v8OBBLoss.__call__ and .preprocess do to a batch (loss.py:621-664) ------------------------------------------
def table_from_labels(labels, batch_size, hw, mut=()):
    """fp32 (B, n_max, 6) rows [cls, x, y, w, h, r]: the tiny-box filter multiplies the WIDTH by the image HEIGHT and the height by the
    width (imgsz is (h, w), loss.py:660), xywh are then scaled by (w, h, w, h), r stays."""
    H, W = np.float32(hw[0]), np.float32(hw[1])
    bi = np.asarray(labels["batch_idx"], np.float32).reshape(-1)
    cls = np.asarray(labels["cls"], np.float32).reshape(-1)
    bb = np.asarray(labels["bboxes"], np.float32).reshape(-1, 5)
    rw, rh = bb[:, 2] * (W if "w_times_w" in mut else H), bb[:, 3] * W
    keep = (rw >= 2) & (rh >= 2)
    bi, cls, bb = bi[keep], cls[keep], bb[keep].copy()
    bb[:, :4] *= np.array([W, H, W, H], np.float32)
    counts = [int((bi == j).sum()) for j in range(batch_size)]
    out = np.zeros((batch_size, max(counts, default=0), 6), np.float32)
    for j in range(batch_size):
        m = bi == j
        out[j, : counts[j], 0], out[j, : counts[j], 1:] = cls[m], bb[m]
    return torch.from_numpy(out)


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------
def _cov(w, h, r):
    a, b, c, s = w * w / 12, h * h / 12, torch.cos(r), torch.sin(r)
    return a * c * c + b * s * s, a * s * s + b * c * c, (a - b) * c * s


def probiou64(o1, o2, eps=1e-7):
    """metrics.py:217-233 on (..., 5) xywhr."""
    x1, y1, x2, y2 = o1[..., 0], o1[..., 1], o2[..., 0], o2[..., 1]
    a1, b1, c1 = _cov(o1[..., 2], o1[..., 3], o1[..., 4])
    a2, b2, c2 = _cov(o2[..., 2], o2[..., 3], o2[..., 4])
    det = (a1 + a2) * (b1 + b2) - (c1 + c2) ** 2
    t1 = ((a1 + a2) * (y1 - y2) ** 2 + (b1 + b2) * (x1 - x2) ** 2) / (det + eps) * 0.25
    t2 = ((c1 + c2) * (x2 - x1) * (y1 - y2)) / (det + eps) * 0.5
    t3 = (det / (4 * ((a1 * b1 - c1 ** 2).clamp(min=0) * (a2 * b2 - c2 ** 2).clamp(min=0)).sqrt() + eps) + eps).log() * 0.5
    bd = (t1 + t2 + t3).clamp(eps, 100.0)
    return 1 - (1 - (-bd).exp() + eps).sqrt()


def _decode(f64, a64, strides, nc, mut=()):
    B = f64[0].shape[0]
    cat = torch.cat([f.reshape(B, 4 * REG + nc, -1) for f in f64], 2).permute(0, 2, 1)  # (B, A, no)
    z = torch.cat([a[:, 0].reshape(B, -1) for a in a64], 1)  # (B, A)
    distri, scores = cat[..., : 4 * REG], cat[..., 4 * REG :]
    ap, st = LU._anchors(f64, strides)
    dist = distri.reshape(B, -1, 4, REG).softmax(3) @ torch.arange(REG, dtype=torch.float64)
    th = (z.sigmoid() - 0.25) * math.pi  # head.py:222
    c, s = th.cos(), th.sin()
    if "angle_centre_route_dropped" in mut:
        c, s = c.detach(), s.detach()
    xf, yf = (dist[..., 2] - dist[..., 0]) / 2, (dist[..., 3] - dist[..., 1]) / 2
    pred = torch.stack((xf * c - yf * s + ap[:, 0], xf * s + yf * c + ap[:, 1], dist[..., 0] + dist[..., 2], dist[..., 1] + dist[..., 3], th), -1)  # grid units
    return cat, distri, scores, ap, st, pred


def _corners(box):
    """a, ab, ad of xywhr2xyxyxyxy (ops.py:589-600) as tal.py:318-322 takes them."""
    ctr, w, h, r = box[..., :2], box[..., 2:3], box[..., 3:4], box[..., 4:5]
    c, s = r.cos(), r.sin()
    v1, v2 = torch.cat((w / 2 * c, w / 2 * s), -1), torch.cat((-h / 2 * s, h / 2 * c), -1)
    a, b, d = ctr + v1 + v2, ctr + v1 - v2, ctr - v1 + v2
    return a, b - a, d - a


def inbox32(feats, gt, strides):
    """The in-box test in fp32 in the reference's order of operations (ops.py:589-600, tal.py:318-330), as csrc/obb_loss.hip states it with
    contraction off: (B, G, A) bool, mask_gt applied.  Plain numpy; equals the reference's own mask on every case (test_obb_loss_host.py)."""
    f, g = np.float32, gt.numpy().astype(np.float32)
    x, y, w, h, r = (g[..., i] for i in range(1, 6))
    cs, sn = np.cos(r), np.sin(r)
    v1x, v1y, v2x, v2y = (w / f(2)) * cs, (w / f(2)) * sn, ((-h) / f(2)) * sn, (h / f(2)) * cs
    ax, ay = (x + v1x) + v2x, (y + v1y) + v2y
    abx, aby, adx, ady = ((x + v1x) - v2x) - ax, ((y + v1y) - v2y) - ay, ((x - v1x) + v2x) - ax, ((y - v1y) + v2y) - ay
    nab, nad = abx * abx + aby * aby, adx * adx + ady * ady
    ap, st = LU._anchors(feats, strides)
    c = (ap * st[:, None]).numpy().astype(np.float32)
    apx, apy = c[None, None, :, 0] - ax[..., None], c[None, None, :, 1] - ay[..., None]
    dab, dad = apx * abx[..., None] + apy * aby[..., None], apx * adx[..., None] + apy * ady[..., None]
    valid = ((((x + y) + w) + h) + r) > 0
    return torch.from_numpy((dab >= 0) & (dab <= nab[..., None]) & (dad >= 0) & (dad <= nad[..., None]) & valid[..., None])


def _pairs(feats, angles, gt, strides, nc, mut=(), delta=DELTA, inbox_mask=None):
    f64, a64 = [f.detach().double() for f in feats], [a.detach().double() for a in angles]
    _, _, scores, ap, st, pred = _decode(f64, a64, strides, nc, mut)
    g = gt.double()
    box = g[..., 1:6]
    valid = (box[..., :4] if "mask_gt_on_xywh" in mut else box).sum(-1) > 0  # loss.py:664
    a, ab, ad = _corners(box)
    cen = ap * st[:, None]
    apv = cen[None, None] - a[:, :, None]  # (B, G, A, 2)
    dab, dad = (apv * ab[:, :, None]).sum(-1), (apv * ad[:, :, None]).sum(-1)
    nab, nad = (ab * ab).sum(-1)[..., None], (ad * ad).sum(-1)[..., None]
    slack = torch.stack((dab / nab, (nab - dab) / nab, dad / nad, (nad - dad) / nad), -1)  # >= 0: the inequality holds
    inbox = ((slack > 0) if "inbox_strict" in mut else (slack >= 0)).all(-1) & valid[..., None]
    near = (slack != 0) & (slack.abs() < delta)
    edge = near.any(-1) & ((slack >= 0) | near).all(-1) & valid[..., None]
    near64 = int(edge.sum())
    if inbox_mask is not None:  # membership pinned by the fp32 arithmetic: nothing about it is unsure
        inbox, edge = inbox_mask & valid[..., None], torch.zeros_like(edge)
    cls = g[..., 0].long().clamp(0, nc - 1)
    ppx = torch.cat((pred[..., :4] * st[None, :, None], pred[..., 4:]), -1)
    ov = probiou64(box[:, :, None, :], ppx[:, None])
    if "overlap_unclamped" not in mut:
        ov = ov.clamp(min=0)
    sc = torch.gather(scores.sigmoid().permute(0, 2, 1), 1, cls[..., None].expand(-1, -1, scores.shape[1]))
    raw_metric = sc.pow(0.5) * ov.pow(6.0)
    return dict(inbox=inbox, edge=edge, overlap=torch.where(inbox, ov, torch.zeros_like(ov)), metric=torch.where(inbox, raw_metric, torch.zeros_like(ov)),
                raw_overlap=ov, raw_metric=raw_metric, cls=cls, valid=valid, near64=near64)


def assign64_rot(feats, angles, gt, strides, nc, topk=10, mut=(), delta=DELTA, inbox_mask=None):
    """owner (B, A) int64 (-1 background); metric, overlap, inbox (B, G, A); ranked / picks / claims / pickers as tests/_loss_util.assign64;
    unsure (B, A) bool with ``kinds`` = anchors per kind (a, b, c); allowed[(b, a)] = the owners an unsure anchor may have.  ``inbox_mask``
    (``inbox32``): membership is taken from it instead of the float64 inequalities, and kind (c) is then empty."""
    p = _pairs(feats, angles, gt, strides, nc, mut, delta, inbox_mask)
    metric, ov = p["metric"], p["overlap"]
    B, G, A = metric.shape
    k_eff = topk - 1 if "topk_minus_1" in mut else topk
    ranked = [[None] * G for _ in range(B)]
    pickers = torch.zeros(B, G, A, dtype=torch.bool)
    ua, ub, uc = (torch.zeros(B, A, dtype=torch.bool) for _ in range(3))
    near = {}
    for b in range(B):
        for g in range(G):
            m = metric[b, g]
            order = torch.sort(m, descending=True, stable=True).indices
            order = order[m[order] > 0]
            ranked[b][g] = order
            pickers[b, g, order[:k_eff]] = True
            if len(order) > topk:
                hi, lo = float(m[order[topk - 1]]), float(m[order[topk]])
                if 0 < (hi - lo) / hi < delta:
                    for a in (int(order[topk - 1]), int(order[topk])):
                        ua[b, a] = True
                        near.setdefault((b, a), []).append(g)
            E = p["edge"][b, g]
            if bool(E.any()):  # kind (c): the edge anchors themselves, and whoever crosses the top-k boundary when they count or do not
                mm = torch.where(E, p["raw_metric"][b, g], m)
                full = torch.sort(mm, descending=True, stable=True).indices
                full = full[mm[full] > 0]
                before = torch.cumsum(E[full].long(), 0) - E[full].long()
                rank = torch.arange(len(full))
                moved = (~E[full]) & (rank >= topk) & (rank - before < topk)  # picked if none of the edge anchors counts, not picked if all do
                for a in E.nonzero().flatten().tolist() + full[moved].tolist():
                    uc[b, a] = True
                    near.setdefault((b, a), []).append(g)
    claims = pickers.sum(1)
    if G:
        mx = ov.amax(1, keepdim=True)
        ids = torch.arange(G)[None, :, None].expand(B, G, A)
        best = torch.where(ov == mx, ids, torch.full_like(ids, -1)).amax(1) if "last_tie" in mut else torch.where(ov == mx, ids, torch.full_like(ids, G)).amin(1)
        single = pickers.int().argmax(1)
        owner = torch.where(claims > 1, best, torch.where(claims == 1, single, torch.full_like(single, -1)))
        if G > 1:
            top2 = ov.topk(2, dim=1).values
            gap = (top2[:, 0] - top2[:, 1]) / top2[:, 0].clamp(min=1e-300)
            ub |= (claims > 1) & (gap > 0) & (gap < delta)
    else:
        owner = torch.full((B, A), -1, dtype=torch.int64)
    unsure = ua | ub | uc
    allowed = {}
    for b, a in unsure.nonzero().tolist():
        s = {int(owner[b, a]), -1, *near.get((b, a), [])}
        if G > 1:
            s |= set(p["raw_overlap"][b, :, a].topk(2).indices.tolist()) | set(p["edge"][b, :, a].nonzero().flatten().tolist())
        allowed[(b, a)] = s
    return dict(owner=owner, metric=metric, overlap=ov, inbox=p["inbox"], edge=p["edge"], ranked=ranked, picks=[[r[:k_eff] for r in row] for row in ranked],
                claims=claims, pickers=pickers, unsure=unsure, kinds=(int(ua.sum()), int(ub.sum()), int(uc.sum())), allowed=allowed, cls=p["cls"], near64=p["near64"])


def loss_from_owner64_rot(feats, angles, gt, owner, strides, nc, gains=GAINS, mut=(), want_grad=True):
    """items (3,), total, head grads, angle grads (lists like the inputs, or None), info -- float64 -- under the given owner map (B, A)."""
    p = _pairs(feats, angles, gt, strides, nc, mut)
    f64 = [f.detach().double().requires_grad_(want_grad) for f in feats]
    a64 = [a.detach().double().requires_grad_(want_grad) for a in angles]
    cat, distri, scores, ap, st, pred = _decode(f64, a64, strides, nc, mut)
    B, G, A = p["metric"].shape
    box = gt.double()[..., 1:6]
    bi, ai = (owner >= 0).nonzero(as_tuple=True)
    gi = owner[bi, ai]
    info = dict(n_fg=int(bi.numel()), mean_iou=float("nan"), clamp_hits=0)
    target = torch.zeros(B, A, nc, dtype=torch.float64)
    l_box = l_dfl = torch.zeros((), dtype=torch.float64)
    t = torch.zeros(0, dtype=torch.float64)
    if bi.numel():
        m, o = p["raw_metric"][bi, gi, ai], p["raw_overlap"][bi, gi, ai]
        max_m = torch.zeros(B * G, dtype=torch.float64).scatter_reduce(0, bi * G + gi, m, "amax")
        max_o = torch.zeros(B * G, dtype=torch.float64).scatter_reduce(0, bi * G + gi, o, "amax")
        t = m * max_o[bi * G + gi] / (max_m[bi * G + gi] + 1e-9)  # tal.py:110-116
        target[bi, ai, p["cls"][bi, gi]] = t
    tss = max(float(t.sum()), 1.0)
    info["tss"] = tss
    l_cls = F.binary_cross_entropy_with_logits(scores, target, reduction="none").sum() / tss
    if bi.numel():
        sa = st[ai, None]
        tb = torch.cat((box[bi, gi, :4] / sa, box[bi, gi, 4:]), 1)  # loss.py:697: grid units, the angle unscaled
        pb = pred[bi, ai]
        if "pixel_units_in_loss" in mut:
            iou = probiou64(torch.cat((pb[:, :4] * sa, pb[:, 4:]), 1), torch.cat((tb[:, :4] * sa, tb[:, 4:]), 1))
        else:
            iou = probiou64(pb, tb)
        l_box = ((1.0 - iou) * t).sum() / tss
        if "dfl_rotated_target" in mut:  # the rotated rectangle's hull instead of the box of the target's xywh
            c, s = tb[:, 4].cos().abs(), tb[:, 4].sin().abs()
            half = torch.stack((tb[:, 2] * c + tb[:, 3] * s, tb[:, 2] * s + tb[:, 3] * c), 1) / 2
        else:
            half = tb[:, 2:4] / 2
        raw = torch.cat((ap[ai] - (tb[:, :2] - half), (tb[:, :2] + half) - ap[ai]), 1)  # loss.py:131
        info["mean_iou"], info["clamp_hits"] = float(iou.detach().mean()), int((raw > CLAMP).sum())
        q = distri[bi, ai].reshape(-1, 4, REG)
        lse = q.logsumexp(-1)
        tv = raw.clamp(0, CLAMP)
        tl = tv.long()
        ql, qr = q.gather(2, tl[..., None]).squeeze(-1), q.gather(2, tl[..., None] + 1).squeeze(-1)
        wl = (tl + 1).double() - tv
        l_dfl = ((((lse - ql) * wl + (lse - qr) * (1 - wl)).mean(-1)) * t).sum() / tss
    items = torch.stack((l_box * gains[0], l_cls * gains[1], l_dfl * gains[2]))
    total = items.sum() * B
    grads = agrads = None
    if want_grad:
        gs = torch.autograd.grad(total, f64 + a64, allow_unused=True)
        gs = [g if g is not None else torch.zeros_like(x) for g, x in zip(gs, f64 + a64)]
        grads, agrads = gs[: len(f64)], gs[len(f64) :]
    return items.detach(), total.detach(), grads, agrads, info


# ---- the real reference's fp32 results (golden file) and the bars ------------------------------------------------------------------
@lru_cache(maxsize=None)
def _golden_file():
    return dict(np.load(GOLDEN))


def golden(cid):
    """items (3,), total, grads / agrads (lists or None), owner (B, A) (-1 where the target score is 0), fg, tscore, overlap / metric (B, G, A),
    gt: the real reference's fp32 run on the case (tools/make_obb_loss_golden.py)."""
    z, pre = _golden_file(), f"{cid}/"
    get = lambda k: torch.from_numpy(z[pre + k])  # noqa: E731
    case = build_case(cid)
    n = len(case["feats"])
    has_grad = pre + "g0" in z
    return dict(items=get("items"), total=get("total"), owner=get("owner").long(), fg=get("fg").bool(), tscore=get("tscore"), overlap=get("overlap"), metric=get("metric"),
                gt=get("gt"), grads=[get(f"g{i}") for i in range(n)] if has_grad else None, agrads=[get(f"ga{i}") for i in range(n)] if has_grad else None)


def item_err(got, ref):
    return LU.item_err(got, ref)


def grad_err(got, ref):
    return LU.grad_err(got, ref)


def pair_err(cid):
    """Largest relative difference of overlap and metric between the real reference (fp32) and float64 over the in-box pairs with a positive metric."""
    case, asg, g32, _ = case_reference(cid)
    sel = asg["inbox"] & (asg["metric"] > 0) & ~asg["edge"]
    if not bool(sel.any()):
        return 0.0
    eo = ((g32["overlap"].double() - asg["overlap"]).abs() / asg["overlap"].clamp(min=1e-300))[sel].max()
    em = ((g32["metric"].double() - asg["metric"]).abs() / asg["metric"].clamp(min=1e-300))[sel].max()
    return float(max(eo, em))


@lru_cache(maxsize=None)
def case_reference(cid):
    """(case, assign64_rot result, golden, bars): computed once per case and shared; callers leave it unchanged."""
    case = build_case(cid)
    asg = assign64_rot(case["feats"], case["angles"], case["gt"], case["strides"], case["nc"], case["topk"], inbox_mask=inbox32(case["feats"], case["gt"], case["strides"]))
    g32 = golden(cid)
    items, total, grads, agrads, _ = loss_from_owner64_rot(case["feats"], case["angles"], case["gt"], g32["owner"], case["strides"], case["nc"], want_grad=case["grad"])
    e_items = item_err(torch.cat((g32["items"], g32["total"].view(1))), torch.cat((items, total.view(1))))
    e_grad = grad_err(g32["grads"] + g32["agrads"], grads + agrads) if case["grad"] else 0.0
    bars = dict(oracle_items=e_items, oracle_grad=e_grad, items=min(ITEM_CEIL, FACTOR * max(e_items, F32_EPS)), grad=min(GRAD_CEIL, FACTOR * max(e_grad, F32_EPS)))
    return case, asg, g32, bars


def owner_errors(owner, asg):
    return LU.owner_errors(owner, asg)


def check_case(cid, owner, out, grads, agrads):
    """The GPU test's checks on one result (owner (B, A), out[4], head and angle gradients or None): a dict of figures and ``ok``."""
    case, asg, _, bars = case_reference(cid)
    owner = owner.cpu().long()
    if tuple(owner.shape) != tuple(asg["owner"].shape):
        outside, inside = int(owner.numel()), 0
        owner_ref = asg["owner"]
    else:
        outside, inside = owner_errors(owner, asg)
        owner_ref = owner
    G = case["gt"].shape[1]
    usable = bool(((owner_ref >= -1) & (owner_ref < max(G, 1))).all()) and (G > 0 or bool((owner_ref < 0).all()))
    items, total, rg, rag, _ = loss_from_owner64_rot(case["feats"], case["angles"], case["gt"], owner_ref if usable else asg["owner"], case["strides"], case["nc"],
                                                     want_grad=grads is not None)
    out = torch.as_tensor(out).detach().cpu().double()
    e_items = item_err(out, torch.cat((items, total.view(1)))) if bool(torch.isfinite(out).all()) else float("inf")
    e_grad = grad_err(list(grads) + list(agrads), rg + rag) if grads is not None else 0.0
    e_head = grad_err(list(grads), rg) if grads is not None else 0.0
    e_angle = grad_err(list(agrads), rag) if grads is not None else 0.0
    res = dict(fg=int((owner >= 0).sum()), unsure=int(asg["unsure"].sum()), owner_wrong=outside, unsure_wrong=inside, oracle_items=bars["oracle_items"],
               items_err=e_items, items_bar=bars["items"], oracle_grad=bars["oracle_grad"], grad_err=e_grad, head_grad_err=e_head, angle_grad_err=e_angle, grad_bar=bars["grad"])
    res["ok_owner"] = outside == 0 and inside == 0
    res["ok_items"] = e_items <= bars["items"]
    res["ok_grad"] = e_grad <= bars["grad"]
    res["ok"] = res["ok_owner"] and res["ok_items"] and res["ok_grad"]
    return res


def mutant_result(cid, mut):
    """What a kernel (or a criterion) with the named defect would return on the case: (owner, out[4], grads, agrads)."""
    case = build_case(cid)
    mut = (mut,)
    gt = table_from_labels(case["labels"], case["feats"][0].shape[0], case["hw"], mut) if case["labels"] is not None else case["gt"]
    owner = assign64_rot(case["feats"], case["angles"], gt, case["strides"], case["nc"], case["topk"], mut=mut)["owner"]
    items, total, grads, agrads, _ = loss_from_owner64_rot(case["feats"], case["angles"], gt, owner, case["strides"], case["nc"], mut=mut, want_grad=case["grad"])
    return owner, torch.cat((items, total.view(1))), grads, agrads


# ---- cases -------------------------------------------------------------------------------------------------------------------
def _table(images):
    """list (per image) of rows [cls, x, y, w, h, r] (None = a zero row) -> (B, gmax, 6) fp32, zero padded."""
    gmax = max((len(r) for r in images), default=0)
    gt = torch.zeros(len(images), gmax, 6, dtype=torch.float32)
    for b, rows in enumerate(images):
        for g, r in enumerate(rows):
            if r is not None:
                gt[b, g] = torch.as_tensor(r, dtype=torch.float32)
    return gt


def _rand_heads(seed, B, nc, hw, strides):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(B, 4 * REG + nc, int(hw[0] // s), int(hw[1] // s), generator=g) * 1.5 for s in strides]
    angles = [torch.randn(B, 1, int(hw[0] // s), int(hw[1] // s), generator=g) * 1.5 for s in strides]
    return feats, angles


def _converged_heads(seed, gt, nc, hw, strides, kappa=4.0, jit=0.05):
    """Random heads, and for every anchor whose centre lies in a label the smallest such label's converged row: the (l, t, r, b) that
    dist2rbox maps onto the label at the label's angle (DFL logits -kappa (i - d)^2, d jittered by 5 %), the angle logit at the label's
    angle (moved into [-pi/4, 3 pi/4) by multiples of pi; + 0.1 N(0,1)), class logit 3 + N(0,1) at the label's class, -4 + 1.5 N(0,1) elsewhere."""
    B = gt.shape[0]
    feats, angles = _rand_heads(seed, B, nc, hw, strides)
    g = torch.Generator().manual_seed(seed + 1000)
    bins = torch.arange(REG, dtype=torch.float32)
    box = gt[..., 1:6].double()
    valid = box.sum(-1) > 0
    a, ab, ad = _corners(box)
    for f, an, s in zip(feats, angles, strides):
        h, w = f.shape[2:]
        cy, cx = torch.meshgrid((torch.arange(h) + 0.5) * s, (torch.arange(w) + 0.5) * s, indexing="ij")
        cen = torch.stack((cx, cy), -1).double()
        for b in range(B):
            if box.shape[1] == 0:
                continue
            apv = cen[None] - a[b, :, None, None]
            dab, dad = (apv * ab[b, :, None, None]).sum(-1), (apv * ad[b, :, None, None]).sum(-1)
            inside = (dab >= 0) & (dab <= (ab[b] ** 2).sum(-1)[:, None, None]) & (dad >= 0) & (dad <= (ad[b] ** 2).sum(-1)[:, None, None]) & valid[b, :, None, None]
            area = (box[b, :, 2] * box[b, :, 3])[:, None, None].expand_as(inside)
            best = torch.where(inside, area, torch.full_like(area, float("inf"))).argmin(0)
            for y, x in inside.any(0).nonzero().tolist():
                gi = int(best[y, x])
                bx, by, bw, bh, r = box[b, gi].tolist()
                while r >= 0.75 * math.pi:
                    r -= math.pi
                while r < -0.25 * math.pi:
                    r += math.pi
                dx, dy = (bx - float(cx[y, x])) / s, (by - float(cy[y, x])) / s
                xf, yf = dx * math.cos(r) + dy * math.sin(r), -dx * math.sin(r) + dy * math.cos(r)
                tgt = torch.tensor([bw / s / 2 - xf, bh / s / 2 - yf, bw / s / 2 + xf, bh / s / 2 + yf]).clamp(0, CLAMP).float() * (1 + jit * torch.randn(4, generator=g))
                f[b, : 4 * REG, y, x] = (-kappa * (bins[None] - tgt[:, None]) ** 2).flatten()
                cl = -4 + 1.5 * torch.randn(nc, generator=g)
                cl[int(gt[b, gi, 0])] = 3 + float(torch.randn(1, generator=g))
                f[b, 4 * REG :, y, x] = cl
                pr = min(max(r / math.pi + 0.25, 0.02), 0.98)
                an[b, 0, y, x] = math.log(pr / (1 - pr)) + 0.1 * float(torch.randn(1, generator=g))
    return feats, angles


def _rand_rboxes(seed, n, nc, hw, lo=0.15, hi=0.6, classes=None):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    u = lambda: float(torch.rand(1, generator=g))  # noqa: E731
    rows = []
    for i in range(n):
        bw, bh = (lo + (hi - lo) * u()) * W, (lo + (hi - lo) * u()) * H
        x, y = (0.15 + 0.7 * u()) * W, (0.15 + 0.7 * u()) * H
        r = (u() - 0.25) * math.pi
        c = classes[i % len(classes)] if classes else int(torch.randint(0, nc, (1,), generator=g))
        rows.append([c, x, y, bw, bh, r])
    return rows


def _labels_from_rows(images, hw):
    """Normalised batch dict (batch_idx, cls, bboxes (M, 5) xywhr) of per-image pixel rows, as a dataset hands it to the criterion."""
    H, W = hw
    bi, cls, bb = [], [], []
    for b, rows in enumerate(images):
        for c, x, y, w, h, r in rows:
            bi.append(float(b)), cls.append([float(c)]), bb.append([x / W, y / H, w / W, h / H, r])
    return {"batch_idx": torch.tensor(bi, dtype=torch.float32), "cls": torch.tensor(cls, dtype=torch.float32).reshape(-1, 1),
            "bboxes": torch.tensor(bb, dtype=torch.float32).reshape(-1, 5)}


# per case id, where other seeds than the defaults were needed to keep the unsure set empty (tools/make_obb_loss_golden.py --seeds): _LSEEDS moves the
# seeds of the random labels (kind (c) depends on the labels alone), _SEEDS replaces the head seed (kinds (a) and (b))
_LSEEDS = {"rand": 6, "conv": 17, "crowd": 7, "nc1": 1, "nc80": 3, "big": 5}
_SEEDS = {"conv": 1, "wrap": 1}


def _ls(cid, base):
    return base + 100 * _LSEEDS.get(cid, 0)


def _std(cid, gt, kind, nc=10, hw=HW, strides=S3, topk=10, grad=True, heads=None, labels=None, device_table=False):
    seed = _SEEDS.get(cid, 100 + sum(map(ord, cid)))
    if heads is None:
        heads = _rand_heads(seed, gt.shape[0], nc, hw, strides) if kind == "R" else _converged_heads(seed, gt, nc, hw, strides)
    return dict(id=cid, feats=heads[0], angles=heads[1], gt=gt, strides=list(strides), nc=nc, topk=topk, hw=hw, grad=grad, kind=kind, labels=labels, device_table=device_table,
                seed=seed)


EDGE_ROWS_0 = [[1, 36.0, 28.0, 48.0, 16.0, 0.0], [4, 56.0, 32.0, 32.0, 32.0, 0.0]]  # x 12..60, y 20..36: stride-8 centres on all four edges and corners; x 40..72, y 16..48: stride-16 / -32 centres
EDGE_ROWS_90 = [[2, 36.0, 28.0, 16.0, 48.0, PI32 / 2], [7, 56.0, 32.0, 32.0, 32.0, PI32 / 2]]  # the same footprints through r = pi/2
TINY_ROWS = [  # (row in pixels, kept by the reference): the filter compares w / W * H and h / H * W with 2 on a 64 x 96 image
    ([1, 20.0, 20.0, 2.5, 10.0, 0.0], False),   # w 2.5 px: 2.5 / 96 * 64 = 1.67 < 2, dropped ONLY because the width meets the height
    ([2, 44.0, 20.0, 10.0, 1.5, 0.0], True),    # h 1.5 px: 1.5 / 64 * 96 = 2.25 >= 2, kept ONLY because the height meets the width
    ([3, 68.0, 20.0, 3.5, 3.5, 0.3], True),     # 3.5 / 96 * 64 = 2.33
    ([4, 20.0, 44.0, 10.0, 1.2, 0.0], False),   # 1.2 / 64 * 96 = 1.8
    ([5, 44.0, 44.0, 1.0, 1.0, 0.0], False),
    ([6, 68.0, 44.0, 30.0, 20.0, 0.6], True),
]


def _tiny_case(cid):
    """Image 0: TINY_ROWS.  Image 1: a 3.25 x 2.5 px label on the stride-8 centre (12, 12) with a prediction of 0.01 cells a side on that
    anchor: 4 sqrt(d1 d2) is of the order of probiou's eps in grid units and 4096 times it in pixels, which is where a box loss in pixels shows."""
    rows = [[r for r, _ in TINY_ROWS], [[8, 12.0, 12.0, 3.25, 2.5, 0.0]]]
    labels = _labels_from_rows(rows, HW)
    gt = table_from_labels(labels, 2, HW)
    feats, angles = _rand_heads(_SEEDS.get(cid, 88), 2, 10, HW, S3)
    feats[0][1, : 4 * REG, 1, 1] = torch.tensor([0.0, math.log(0.005)] + [-30.0] * 14).repeat(4)
    feats[0][1, 4 * REG :, 1, 1] = -4.0
    feats[0][1, 4 * REG + 8, 1, 1] = 3.0
    angles[0][1, 0, 1, 1] = math.log(0.25 / 0.75)  # theta = 0
    return _std(cid, gt, "built", heads=(feats, angles), labels=labels)


def _negsum_case(cid):
    """A 6 x 6 px label at (3, 3) with r = -18.5: x + y + w + h = 18, with r the sum is -0.5, so mask_gt treats the row like padding although its
    rectangle holds the stride-8 centre (4, 4) at any angle.  The other labels keep their anchors."""
    rows = [[[3, 3.0, 3.0, 6.0, 6.0, -18.5], [5, 60.0, 30.0, 40.0, 24.0, 0.4]], [[7, 30.0, 34.0, 30.0, 30.0, -0.5]]]
    labels = _labels_from_rows(rows, HW)
    return _std(cid, table_from_labels(labels, 2, HW), "R", labels=labels)


def _clampov_case(cid):
    """A 200 x 200 px label centred 95 px left of the image holds the eight stride-8 centres of the first column only; three of them predict a
    zero-size box (all sides one-hot at bin 0): ProbIoU is then 1 - sqrt(1 + eps - exp(-bd)) with bd > 16.2, a NEGATIVE number that clamp(0)
    makes 0 -- metric 0, never picked.  Without the clamp its sixth power is a positive metric and the three anchors are taken.  Value only: the
    reference's own backward gives NaN at a zero-size box."""
    gt = _table([[[2, -95.0, 32.0, 200.0, 200.0, 0.0], [6, 60.0, 30.0, 36.0, 28.0, 0.7]], [[1, 40.0, 30.0, 40.0, 30.0, 1.0]]])
    feats, angles = _rand_heads(_SEEDS.get(cid, 66), 2, 10, HW, S3)
    onehot0 = torch.where(torch.arange(REG) == 0, 40.0, 0.0).repeat(4)
    for y in (1, 4, 6):
        feats[0][0, : 4 * REG, y, 0] = onehot0
    return _std(cid, gt, "built", heads=(feats, angles), grad=False)


def build_case(cid):
    if cid == "rand":
        return _std(cid, _table([_rand_rboxes(_ls(cid, 11), 4, 10, HW), _rand_rboxes(_ls(cid, 12), 3, 10, HW), _rand_rboxes(_ls(cid, 13), 5, 10, HW)]), "R")
    if cid == "conv":
        return _std(cid, _table([_rand_rboxes(_ls(cid, 21), 4, 10, HW), _rand_rboxes(_ls(cid, 22), 3, 10, HW)]), "C", strides=S4)
    if cid == "edge":
        return _std(cid, _table([EDGE_ROWS_0, EDGE_ROWS_90]), "R")
    if cid == "thin":
        q = PI32 / 4
        return _std(cid, _table([[[3, 44.0, 28.0, 60.0, 3.0, q], [5, 52.0, 36.0, 3.0, 60.0, q]], [[0, 36.0, 36.0, 3.0, 60.0, -q + 0.01], [9, 60.0, 28.0, 60.0, 3.0, q + 0.02]]]), "R")
    if cid == "dup":
        a, c = [3, 40.0, 30.0, 40.0, 30.0, 0.5], [2, 48.0, 32.0, 50.0, 14.0, 0.3]
        return _std(cid, _table([[a, a, c, [6] + c[1:5] + [0.3 + PI32 / 2]], [[2] + a[1:], [5] + a[1:]]]), "C")
    if cid == "crowd":
        return _std(cid, _table([_rand_rboxes(_ls(cid, 31), 40, 10, HW, lo=0.1, hi=0.35), []]), "C")
    if cid == "none":
        return _std(cid, torch.zeros(2, 0, 6), "R", labels={"batch_idx": torch.zeros(0), "cls": torch.zeros(0, 1), "bboxes": torch.zeros(0, 5)})
    if cid == "tiny":
        return _tiny_case(cid)
    if cid == "negsum":
        return _negsum_case(cid)
    if cid == "wrap":
        hi = float(torch.nextafter(torch.tensor(0.75 * math.pi, dtype=torch.float32), torch.tensor(0.0)))
        return _std(cid, _table([[[1, 30.0, 30.0, 36.0, 20.0, -PI32 / 4], [4, 66.0, 34.0, 30.0, 22.0, hi]], [[8, 48.0, 32.0, 44.0, 18.0, PI32 / 2]]]), "C")
    if cid in ("nc1", "nc80"):
        nc = int(cid[2:])
        return _std(cid, _table([_rand_rboxes(_ls(cid, 41 + nc), 4, nc, HW, classes=[0, nc - 1]), _rand_rboxes(_ls(cid, 42 + nc), 3, nc, HW, classes=[nc - 1, 0])]), "R", nc=nc)
    if cid == "pad":
        rows = _rand_rboxes(_ls(cid, 51), 5, 10, HW)
        return _std(cid, _table([[], [None, rows[0], None, None, rows[1], rows[2], None, None, None, rows[3], None, rows[4], None, None]]), "R", device_table=True)
    if cid == "clampov":
        return _clampov_case(cid)
    if cid == "big":  # 128 x 192 on the P2 strides: the first label's hull holds 1,900 cells, more than the pick kernel keeps in LDS (1,024): its re-evaluating
        hw = (128, 192)  # path; value only.  Axis-aligned with edges 1 px from the nearest anchor centres: a rotated label this long always has anchors within DELTA of an edge
        return _std(cid, _table([[[3, 96.0, 64.0, 178.0, 118.0, 0.0]] + _rand_rboxes(_ls(cid, 61), 2, 10, hw, lo=0.1, hi=0.3), _rand_rboxes(_ls(cid, 62), 3, 10, hw, lo=0.1, hi=0.3)]), "R", hw=hw, strides=S4,
                    grad=False)
    raise KeyError(cid)


CASE_IDS = ["rand", "conv", "edge", "thin", "dup", "crowd", "none", "tiny", "negsum", "wrap", "nc1", "nc80", "pad", "clampov", "big"]
