"""Label-geometry and converged-head sweep of the detection loss (``dy_detection_loss``): the cases, a dense float64 reference and the
checks, shared by tests/test_loss_geometry_host.py (CPU) and tests/test_loss_geometry_gpu.py.  Plain CPU torch; not collected.

The reference follows the maths of oracle/loss_oracle.py (TaskAlignedAssigner + BCE / CIoU / DFL) in float64 on the SAME fp32 box table
and fp32 head maps the device gets, in two halves:

* ``assign64``: the assignment (owner map, per-pair metric and overlap, ranked candidates, claim counts) with the kernel's documented
  deviation (a pick with metric exactly 0 is never taken) and its documented tie rules (equal metrics: ascending anchor index; equal
  overlaps of a shared anchor: first box index);
* ``loss_from_owner64``: everything downstream as a function of an owner map alone, differentiable (float64 autograd, the targets and
  CIoU's alpha detached), so the numeric bars are evaluated under the DEVICE's owner map and one flipped near-tie cannot leak into them.

Unsure set: the only anchors whose owner may differ from ``assign64``'s.  (a) the anchors ranked topk-th and (topk+1)-th of a box when
their float64 metrics differ by a non-zero relative gap below DELTA; (b) an anchor claimed by two or more boxes whose two largest float64
overlaps over all boxes differ by a non-zero relative gap below DELTA.  Exact ties are pinned, not unsure.

DELTA = 16 * 1.1e-4 = 1.76e-3.  MEASURED_PAIR_ERR = 1.1e-4 is the largest relative difference between the fp32 oracle's and this
reference's metric or overlap over all in-box pairs with a positive metric of all cases (1.094e-4, case pad-R, the same to eight digits
on two hosts; 5e-5 in edge-R, below that elsewhere); test_loss_geometry_host.py::test_delta_covers_the_float32_oracle_and_the_unsure_
set_is_small measures it again and fails if a case exceeds it.  The largest differences belong to overlaps near 0, where CIoU = iou -
penalty cancels; such pairs do reach top-k boundaries in the random-head cases (metrics down to 1e-23), so they are not left out.  The
factor 16 covers the device's expf / powf / atanf being a few ulp off the host's, amplified by the sixth power.  Head seeds (_SEEDS) are
chosen so that the reference alone leaves the unsure set empty in every case.
"""
from __future__ import annotations

import math
from functools import lru_cache

import torch
import torch.nn.functional as F

from oracle import loss_oracle as LO

MEASURED_PAIR_ERR = 1.1e-4
DELTA = 16 * MEASURED_PAIR_ERR
FACTOR = 16.0
ITEM_CEIL, GRAD_CEIL = 2e-4, 1e-4  # the bars of tests/test_loss_gpu.py stay as ceilings
ITEM_FLOOR = 0.05  # |a - b| / max(|b|, 0.05): never looser than test_loss_gpu.py's rtol 2e-4 + atol 1e-5
F32_EPS = 2.0 ** -23  # an error measured as 0 still leaves the result's own rounding to fp32
REG = 16
GAINS = (7.5, 0.5, 1.5)
CLAMP = float(torch.tensor(REG - 1 - 0.01, dtype=torch.float32))  # what clamp(0, reg_max - 1 - 0.01) does to an fp32 tensor
MUTANTS = ("inbox_ge", "last_tie", "claimants_only", "topk_minus_1", "max_over_picks", "no_dfl_clamp", "swap_hw", "alpha_attached", "box_pixels")


# ---- float64 reference ---------------------------------------------------------------------------------------------------------
def _anchors(feats, strides, swap_hw=False):
    pts, st = [], []
    for f, s in zip(feats, strides):
        h, w = f.shape[2:]
        idx = torch.arange(h * w)
        row = h if swap_hw else w  # the mutant divides the anchor index by h
        gy, gx = idx // row, idx % row
        pts.append(torch.stack((gx.double() + 0.5, gy.double() + 0.5), 1))
        st.append(torch.full((h * w,), float(s), dtype=torch.float64))
    return torch.cat(pts), torch.cat(st)


def ciou64(box1, box2, detach_alpha=True, eps=1e-7):
    b1x1, b1y1, b1x2, b1y2 = box1.unbind(-1)
    b2x1, b2y1, b2x2, b2y2 = box2.unbind(-1)
    w1, h1, w2, h2 = b1x2 - b1x1, b1y2 - b1y1 + eps, b2x2 - b2x1, b2y2 - b2y1 + eps
    inter = (torch.minimum(b1x2, b2x2) - torch.maximum(b1x1, b2x1)).clamp(min=0) * (torch.minimum(b1y2, b2y2) - torch.maximum(b1y1, b2y1)).clamp(min=0)
    iou = inter / (w1 * h1 + w2 * h2 - inter + eps)
    cw, ch = torch.maximum(b1x2, b2x2) - torch.minimum(b1x1, b2x1), torch.maximum(b1y2, b2y2) - torch.minimum(b1y1, b2y1)
    c2 = cw ** 2 + ch ** 2 + eps
    rho2 = ((b2x1 + b2x2 - b1x1 - b1x2) ** 2 + (b2y1 + b2y2 - b1y1 - b1y2) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    alpha = v / (v - iou + (1 + eps))
    return iou - (rho2 / c2 + v * (alpha.detach() if detach_alpha else alpha))


def _decode(feats64, strides, nc, mut=()):
    B = feats64[0].shape[0]
    cat = torch.cat([f.reshape(B, 4 * REG + nc, -1) for f in feats64], 2).permute(0, 2, 1)  # (B, A, no)
    distri, scores = cat[..., : 4 * REG], cat[..., 4 * REG :]
    ap, st = _anchors(feats64, strides, "swap_hw" in mut)
    dist = distri.reshape(B, -1, 4, REG).softmax(3) @ torch.arange(REG, dtype=torch.float64)
    pb = torch.cat((ap - dist[..., :2], ap + dist[..., 2:]), -1)  # grid units
    return cat, distri, scores, ap, st, pb


def _pairs(feats, gt, strides, nc, mut=()):
    """Per (image, box, anchor), detached: in-box & valid mask, overlap, metric."""
    f64 = [f.detach().double() for f in feats]
    _, _, scores, ap, st, pb = _decode(f64, strides, nc, mut)
    g = gt.double()
    box = g[..., 1:5]
    valid = box.sum(-1) > 0  # loss.py:229
    c = ap * st[:, None]
    d = torch.stack((c[None, None, :, 0] - box[..., None, 0], c[None, None, :, 1] - box[..., None, 1], box[..., None, 2] - c[None, None, :, 0],
                     box[..., None, 3] - c[None, None, :, 1]), -1).amin(-1)
    inbox = ((d >= 0) if "inbox_ge" in mut else (d > 1e-9)) & valid[..., None]
    cls = g[..., 0].long().clamp(0, nc - 1)
    ov = ciou64(box[:, :, None, :], (pb * st[:, None])[:, None, :, :]).clamp(min=0)
    ov = torch.where(inbox, ov, torch.zeros_like(ov))
    sc = torch.gather(scores.sigmoid().permute(0, 2, 1), 1, cls[..., None].expand(-1, -1, scores.shape[1]))
    metric = torch.where(inbox, sc.pow(0.5) * ov.pow(6.0), torch.zeros_like(ov))
    return dict(inbox=inbox, overlap=ov, metric=metric, cls=cls, valid=valid)


def assign64(feats, gt, strides, nc, topk=10, mut=(), delta=DELTA):
    """owner (B, A) int64 (-1 background); metric, overlap, inbox (B, G, A); ranked[b][g]: the box's positive-metric candidates in
    (metric desc, anchor asc) order; picks[b][g] = its first topk; claims (B, A); pickers (B, G, A) bool; unsure (B, A) bool and
    allowed[(b, a)] = the owners an unsure anchor may have."""
    p = _pairs(feats, gt, strides, nc, mut)
    metric, ov = p["metric"], p["overlap"]
    B, G, A = metric.shape
    k_eff = topk - 1 if "topk_minus_1" in mut else topk
    ranked = [[None] * G for _ in range(B)]
    pickers = torch.zeros(B, G, A, dtype=torch.bool)
    unsure = torch.zeros(B, A, dtype=torch.bool)
    near = {}  # (b, a) -> boxes whose top-k boundary the anchor sits at
    for b in range(B):
        for g in range(G):
            m = metric[b, g]
            order = torch.sort(m, descending=True, stable=True).indices  # stable: equal metrics keep ascending anchor index
            order = order[m[order] > 0]
            ranked[b][g] = order
            pickers[b, g, order[:k_eff]] = True
            if len(order) > topk:
                hi, lo = float(m[order[topk - 1]]), float(m[order[topk]])
                if 0 < (hi - lo) / hi < delta:
                    for a in (int(order[topk - 1]), int(order[topk])):
                        unsure[b, a] = True
                        near.setdefault((b, a), []).append(g)
    claims = pickers.sum(1)
    if G:
        src = torch.where(pickers, ov, torch.full_like(ov, -1.0)) if "claimants_only" in mut else ov
        mx = src.amax(1, keepdim=True)
        ids = torch.arange(G)[None, :, None].expand(B, G, A)
        best = torch.where(src == mx, ids, torch.full_like(ids, -1)).amax(1) if "last_tie" in mut else torch.where(src == mx, ids, torch.full_like(ids, G)).amin(1)
        single = pickers.int().argmax(1)
        owner = torch.where(claims > 1, best, torch.where(claims == 1, single, torch.full_like(single, -1)))
        top2 = ov.topk(min(2, G), dim=1).values
        if G > 1:
            gap = (top2[:, 0] - top2[:, 1]) / top2[:, 0].clamp(min=1e-300)
            unsure |= (claims > 1) & (gap > 0) & (gap < delta)
    else:
        owner = torch.full((B, A), -1, dtype=torch.int64)
    allowed = {}
    for b, a in unsure.nonzero().tolist():
        s = {int(owner[b, a]), -1, *near.get((b, a), [])}
        if G > 1:
            s |= set(ov[b, :, a].topk(2).indices.tolist())
        allowed[(b, a)] = s
    return dict(owner=owner, metric=metric, overlap=ov, inbox=p["inbox"], ranked=ranked, picks=[[r[:k_eff] for r in row] for row in ranked],
                claims=claims, pickers=pickers, unsure=unsure, allowed=allowed, cls=p["cls"])


def loss_from_owner64(feats, gt, owner, strides, nc, topk=10, gains=GAINS, mut=(), want_grad=True):
    """items (3,), total, grads (list like feats, or None), info — all float64 — under the given owner map (B, A)."""
    p = _pairs(feats, gt, strides, nc, mut)
    f64 = [f.detach().double().requires_grad_(want_grad) for f in feats]
    cat, distri, scores, ap, st, pb = _decode(f64, strides, nc, mut)
    B, G, A = p["metric"].shape
    box = gt.double()[..., 1:5]
    bi, ai = (owner >= 0).nonzero(as_tuple=True)
    gi = owner[bi, ai]
    info = dict(n_fg=int(bi.numel()), mean_ciou=float("nan"), clamp_hits=0)
    target = torch.zeros(B, A, nc, dtype=torch.float64)
    l_box = l_dfl = torch.zeros((), dtype=torch.float64)
    t = torch.zeros(0, dtype=torch.float64)
    if bi.numel():
        m, o = p["metric"][bi, gi, ai], p["overlap"][bi, gi, ai]
        if "max_over_picks" in mut:
            pk = assign64(feats, gt, strides, nc, topk, mut)["pickers"]
            max_m, max_o = (p["metric"] * pk).amax(-1).flatten(), (p["overlap"] * pk).amax(-1).flatten()
        else:
            max_m = torch.zeros(B * G, dtype=torch.float64).scatter_reduce(0, bi * G + gi, m, "amax")
            max_o = torch.zeros(B * G, dtype=torch.float64).scatter_reduce(0, bi * G + gi, o, "amax")
        t = m * max_o[bi * G + gi] / (max_m[bi * G + gi] + 1e-9)  # tal.py:110-116
        target[bi, ai, p["cls"][bi, gi]] = t
    tss = max(float(t.sum()), 1.0)
    info["tss"] = tss
    l_cls = F.binary_cross_entropy_with_logits(scores, target, reduction="none").sum() / tss
    if bi.numel():
        sa = st[ai, None]
        tb = box[bi, gi] / sa
        scale = sa if "box_pixels" in mut else 1.0
        iou = ciou64(pb[bi, ai] * scale, tb * scale, detach_alpha="alpha_attached" not in mut)
        l_box = ((1.0 - iou) * t).sum() / tss
        raw = torch.cat((ap[ai] - tb[:, :2], tb[:, 2:] - ap[ai]), 1)
        info["mean_ciou"], info["clamp_hits"] = float(iou.detach().mean()), int((raw > CLAMP).sum())
        q = distri[bi, ai].reshape(-1, 4, REG)
        lse = q.logsumexp(-1)
        if "no_dfl_clamp" in mut:  # what unclamped indices read: the row's next floats, here kept inside the row
            tl = raw.long()
            flat = (torch.arange(4)[None] * REG + tl)
            row = cat[bi, ai]
            ql, qr = row.gather(1, flat.clamp(max=row.shape[1] - 1)), row.gather(1, (flat + 1).clamp(max=row.shape[1] - 1))
            tv = raw
        else:
            tv = raw.clamp(0, CLAMP)
            tl = tv.long()
            ql, qr = q.gather(2, tl[..., None]).squeeze(-1), q.gather(2, tl[..., None] + 1).squeeze(-1)
        wl = (tl + 1).double() - tv
        l_dfl = ((((lse - ql) * wl + (lse - qr) * (1 - wl)).mean(-1)) * t).sum() / tss
    items = torch.stack((l_box * gains[0], l_cls * gains[1], l_dfl * gains[2]))
    total = items.sum() * B
    grads = [g if g is not None else torch.zeros_like(f) for g, f in zip(torch.autograd.grad(total, f64, allow_unused=True), f64)] if want_grad else None
    return items.detach(), total.detach(), grads, info


# ---- the fp32 oracle on a case, and its error against float64 ---------------------------------------------------------------------
def oracle32(case, want_grad=True):
    feats = [f.clone().requires_grad_(want_grad) for f in case["feats"]]
    total, items, asg = LO.v8_detection_loss(feats, None, case["strides"], case["nc"], tal_topk=case["topk"], return_assign=True, targets=case["gt"])
    grads = None
    if want_grad:
        total.backward()
        grads = [f.grad if f.grad is not None else torch.zeros_like(f) for f in feats]
    pos = asg["target_scores"].sum(-1) > 0
    owner = torch.where(pos, asg["target_gt_idx"], torch.full_like(asg["target_gt_idx"], -1))
    return dict(items=items, total=total.detach(), grads=grads, owner=owner, fg=asg["fg_mask"], tscore=asg["target_scores"].sum(-1))


def oracle_pairs32(case):
    """The fp32 oracle's overlap and metric of every (image, box, anchor), by the oracle's own functions (in-box masking left out)."""
    from oracle.drone_yolo_oracle import dist2bbox, make_anchors

    feats, gt, nc = case["feats"], case["gt"], case["nc"]
    B = gt.shape[0]
    pd, ps = torch.cat([f.reshape(B, 4 * REG + nc, -1) for f in feats], 2).split((4 * REG, nc), 1)
    ap, st = make_anchors([f.shape[2:] for f in feats], case["strides"], 0.5)
    dist = pd.permute(0, 2, 1).reshape(B, -1, 4, REG).softmax(3).matmul(torch.arange(REG, dtype=torch.float32))
    ov = LO.bbox_ciou(gt[:, :, None, 1:5], (dist2bbox(dist, ap, xywh=False) * st)[:, None]).squeeze(-1).clamp(min=0)
    sc = ps.sigmoid()[torch.arange(B)[:, None], gt[..., 0].long()]
    return ov, sc.pow(0.5) * ov.pow(6.0)


def pair_err(case, asg):
    """Largest relative difference of overlap and metric between the fp32 oracle and float64 over the in-box pairs with a positive metric."""
    if case["gt"].shape[1] == 0:
        return 0.0
    ov32, m32 = oracle_pairs32(case)
    sel = asg["inbox"] & (asg["metric"] > 0)
    if not bool(sel.any()):
        return 0.0
    eo = ((ov32.double() - asg["overlap"]).abs() / asg["overlap"].clamp(min=1e-300))[sel].max()
    em = ((m32.double() - asg["metric"]).abs() / asg["metric"].clamp(min=1e-300))[sel].max()
    return float(max(eo, em))


def item_err(got, ref):
    got, ref = torch.as_tensor(got).double().flatten(), torch.as_tensor(ref).double().flatten()
    return float(((got - ref).abs() / ref.abs().clamp(min=ITEM_FLOOR)).max())


def grad_err(got, ref):
    """Largest error of any level relative to that level's largest reference entry; inf if an element is not finite."""
    worst = 0.0
    for g, r in zip(got, ref):
        g = g.detach().cpu().double()
        if not bool(torch.isfinite(g).all()):
            return float("inf")
        worst = max(worst, float((g - r).abs().max()) / max(float(r.abs().max()), 1e-30))
    return worst


def owner_errors(owner, asg):
    """(wrong outside the unsure set, wrong inside it): inside, the owner must be one of the candidates."""
    owner = owner.cpu().long()
    diff = owner != asg["owner"]
    outside = int((diff & ~asg["unsure"]).sum())
    inside = sum(1 for (b, a), ok in asg["allowed"].items() if int(owner[b, a]) not in ok)
    return outside, inside


@lru_cache(maxsize=None)
def case_reference(cid):
    """(case, assign64 result, oracle32 result, bars): computed once per case and shared; callers leave it unchanged."""
    case = build_case(cid)
    asg = assign64(case["feats"], case["gt"], case["strides"], case["nc"], case["topk"])
    o32 = oracle32(case, want_grad=case["grad"])
    items, total, grads, _ = loss_from_owner64(case["feats"], case["gt"], o32["owner"], case["strides"], case["nc"], case["topk"], want_grad=case["grad"])
    e_items = item_err(torch.cat((o32["items"], o32["total"].view(1))), torch.cat((items, total.view(1))))
    e_grad = grad_err(o32["grads"], grads) if case["grad"] else 0.0
    bars = dict(oracle_items=e_items, oracle_grad=e_grad, items=min(ITEM_CEIL, FACTOR * max(e_items, F32_EPS)), grad=min(GRAD_CEIL, FACTOR * max(e_grad, F32_EPS)))
    return case, asg, o32, bars


def check_case(cid, owner, out, grads, mut_ref=()):
    """The checks of the GPU test on one result (owner (B, A), out[4], grads or None): a dict of figures and ``ok``."""
    case, asg, _, bars = case_reference(cid)
    owner = owner.cpu().long()
    outside, inside = owner_errors(owner, asg)
    items, total, rgrads, _ = loss_from_owner64(case["feats"], case["gt"], owner, case["strides"], case["nc"], case["topk"], want_grad=grads is not None)
    out = torch.as_tensor(out).detach().cpu().double()
    e_items = item_err(out, torch.cat((items, total.view(1)))) if bool(torch.isfinite(out).all()) else float("inf")
    e_grad = grad_err(grads, rgrads) if grads is not None else 0.0
    res = dict(fg=int((owner >= 0).sum()), unsure=int(asg["unsure"].sum()), owner_wrong=outside, unsure_wrong=inside, oracle_items=bars["oracle_items"],
               items_err=e_items, items_bar=bars["items"], oracle_grad=bars["oracle_grad"], grad_err=e_grad, grad_bar=bars["grad"])
    res["ok_owner"] = outside == 0 and inside == 0
    res["ok_items"] = e_items <= bars["items"]
    res["ok_grad"] = e_grad <= bars["grad"]
    res["ok"] = res["ok_owner"] and res["ok_items"] and res["ok_grad"]
    return res


def mutant_result(cid, mut):
    """What a kernel with the named defect would return on the case: (owner, out[4], grads)."""
    case = build_case(cid)
    mut = (mut,)
    owner = assign64(case["feats"], case["gt"], case["strides"], case["nc"], case["topk"], mut=mut)["owner"]
    items, total, grads, _ = loss_from_owner64(case["feats"], case["gt"], owner, case["strides"], case["nc"], case["topk"], mut=mut, want_grad=case["grad"])
    return owner, torch.cat((items, total.view(1))), grads


def large_box_labels(bs, seed, n=4):
    """``n`` boxes per image of 0.1 .. 0.6 of the image a side: at 64 pixels ``synthetic_labels`` (median size 0.03 = 2 pixels) assigns next to
    nothing -- its (2, 64, 7, 6.0) case has ONE positive anchor and box / DFL terms of 0.0 -- so the 64-pixel cases of tests/test_loss_gpu.py use these."""
    g = torch.Generator().manual_seed(seed)
    wh = torch.rand(bs * n, 2, generator=g) * 0.5 + 0.1
    cxy = wh / 2 + torch.rand(bs * n, 2, generator=g) * (1 - wh)
    return {"batch_idx": torch.arange(bs).repeat_interleave(n).float(), "cls": torch.randint(0, 10, (bs * n, 1), generator=g).float(),
            "bboxes": torch.cat((cxy, wh), 1)}


# ---- cases -------------------------------------------------------------------------------------------------------------------
S4 = (4.0, 8.0, 16.0, 32.0)


def _table(images):
    """list (per image) of rows [cls, x1, y1, x2, y2] (None = a zero row) -> (B, gmax, 5) fp32, zero padded."""
    gmax = max((len(r) for r in images), default=0)
    gt = torch.zeros(len(images), gmax, 5, dtype=torch.float32)
    for b, rows in enumerate(images):
        for g, r in enumerate(rows):
            if r is not None:
                gt[b, g] = torch.as_tensor(r, dtype=torch.float32)
    return gt


def _rand_heads(seed, B, nc, hw, strides):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 4 * REG + nc, int(hw[0] // s), int(hw[1] // s), generator=g) * 1.5 for s in strides]


def _converged_heads(seed, gt, nc, hw, strides, kappa=4.0, jit=0.05):
    """R heads, and for every anchor whose centre lies in a box the smallest such box's converged row: DFL logits -kappa (i - d)^2 with
    d = clamped target distance * (1 + jit N(0,1)), class logit 3 + N(0,1) for the box's class and -4 + 1.5 N(0,1) elsewhere."""
    B = gt.shape[0]
    feats = _rand_heads(seed, B, nc, hw, strides)
    g = torch.Generator().manual_seed(seed + 1000)
    bins = torch.arange(REG, dtype=torch.float32)
    box = gt[..., 1:5]
    area = ((box[..., 2] - box[..., 0]) * (box[..., 3] - box[..., 1])).double()
    valid = box.double().sum(-1) > 0
    for f, s in zip(feats, strides):
        h, w = f.shape[2:]
        cy, cx = torch.meshgrid((torch.arange(h) + 0.5) * s, (torch.arange(w) + 0.5) * s, indexing="ij")
        for b in range(B):
            d = torch.stack((cx[None] - box[b, :, 0, None, None], cy[None] - box[b, :, 1, None, None], box[b, :, 2, None, None] - cx[None],
                             box[b, :, 3, None, None] - cy[None]), -1)  # (G, h, w, 4)
            inside = (d.amin(-1) > 1e-9) & valid[b, :, None, None]
            a = torch.where(inside, area[b, :, None, None].expand_as(inside), torch.full(inside.shape, float("inf"), dtype=torch.float64))
            if a.numel() == 0:
                continue
            best = a.argmin(0)
            for y, x in inside.any(0).nonzero().tolist():
                gi = int(best[y, x])
                tgt = (d[gi, y, x] / s).clamp(0, CLAMP) * (1 + jit * torch.randn(4, generator=g))
                f[b, : 4 * REG, y, x] = (-kappa * (bins[None] - tgt[:, None]) ** 2).flatten()
                cl = -4 + 1.5 * torch.randn(nc, generator=g)
                cl[int(gt[b, gi, 0])] = 3 + float(torch.randn(1, generator=g))
                f[b, 4 * REG :, y, x] = cl
    return feats


def _rand_boxes(seed, n, nc, hw, lo=0.1, hi=0.6, classes=None):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    rows = []
    for i in range(n):
        bw, bh = (lo + (hi - lo) * float(torch.rand(1, generator=g))) * W, (lo + (hi - lo) * float(torch.rand(1, generator=g))) * H
        x1, y1 = float(torch.rand(1, generator=g)) * (W - bw), float(torch.rand(1, generator=g)) * (H - bh)
        c = classes[i % len(classes)] if classes else int(torch.randint(0, nc, (1,), generator=g))
        rows.append([c, x1, y1, x1 + bw, y1 + bh])
    return rows


def _ulp(v, direction):
    t = torch.tensor(v, dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(float("inf") * direction, dtype=torch.float32)))


def _edge_rows(step):
    """One box per stride with every edge on an anchor centre of that stride (x = (g + 0.5) s); step = 0: exactly, +1: every side one
    fp32 ulp inward, -1: one ulp outward."""
    base = [[1, 10.0, 14.0, 38.0, 34.0], [4, 12.0, 20.0, 44.0, 52.0], [7, 8.0, 24.0, 56.0, 40.0], [9, 16.0, 16.0, 48.0, 48.0]]
    if step == 0:
        return base
    return [[c, _ulp(x1, step), _ulp(y1, step), _ulp(x2, -step), _ulp(y2, -step)] for c, x1, y1, x2, y2 in base]


SLIVER_ROWS = [  # (row, in-box candidates over all levels): centres are 2 + 4k, 4 + 8k, 8 + 16k, 16 + 32k
    ([0, 2.5, 2.5, 3.5, 3.5], 0), ([1, 30.5, 3.0, 33.5, 60.0], 0), ([2, 10.5, 20.5, 11.5, 40.0], 0),  # valid, no anchor at any level
    ([3, 9.0, 9.0, 11.0, 11.0], 1), ([4, 11.0, 11.0, 13.0, 13.0], 1), ([5, 7.0, 23.0, 9.0, 25.0], 1), ([6, 15.0, 47.0, 17.0, 49.0], 1),  # one anchor at stride 4 / 8 / 16 / 32
    ([7, 9.0, 37.0, 19.0, 39.0], 3), ([8, 5.0, 53.0, 15.0, 59.0], 7), ([9, 41.0, 5.0, 47.0, 19.0], 9), ([0, 49.0, 33.0, 57.0, 35.0], 2),
]

_SEEDS = {'edge-R': 9, 'edge-C': 3, 'dup-R': 2, 'dup-C': 2, 'crowd-C': 9, 'pad-R': 14, 'rect-R': 1, 'rect-C': 9, 'nc1-R': 2, 'nc80-R': 1, 'lv3-C': 1, 'k13-R': 4}  # per case id, where another seed than the default was needed to keep the unsure set within its cap


def _std(cid, gt, kind, nc=10, hw=(64, 64), strides=S4, topk=10, grad=True, seed=None, feats=None):
    seed = _SEEDS.get(cid, 100 + sum(map(ord, cid))) if seed is None else seed
    if feats is None:
        feats = _rand_heads(seed, gt.shape[0], nc, hw, strides) if kind == "R" else _converged_heads(seed, gt, nc, hw, strides)
    return dict(id=cid, feats=feats, gt=gt, strides=list(strides), nc=nc, topk=topk, hw=hw, grad=grad, kind=kind)


def _peak_case():
    """Base: converged heads.  Then, per box, in-box anchors in turn get: all four sides one-hot at bin 0 (a zero-size prediction), all
    four at bin 15, left/top at 15 with right/bottom at 0, or stay converged; one-hot = logit 30.  Class logits of every fourth anchor
    are +50 at the box's class and -50 elsewhere; of every fourth (offset 1) all -50."""
    gt = _table([[[2, 6.3, 8.1, 39.2, 30.7], [5, 28.4, 33.0, 60.1, 61.2]], [[1, 3.0, 5.0, 33.0, 40.0], [3, 40.5, 38.5, 62.0, 58.0]]])
    feats = _converged_heads(77, gt, 10, (64, 64), S4)
    asg = assign64(feats, gt, S4, 10)
    a0 = 0
    for f in feats:
        h, w = f.shape[2:]
        for b in range(gt.shape[0]):
            for g in range(gt.shape[1]):
                ids = asg["inbox"][b, g, a0 : a0 + h * w].nonzero().flatten().tolist()
                for n, al in enumerate(ids):
                    y, x = al // w, al % w
                    onehot = lambda k: torch.where(torch.arange(REG) == k, 30.0, 0.0)  # noqa: E731
                    if n % 4 == 0:
                        f[b, : 4 * REG, y, x] = onehot(0).repeat(4)
                    elif n % 4 == 1:
                        f[b, : 4 * REG, y, x] = onehot(15).repeat(4)
                    elif n % 4 == 2:
                        f[b, : 4 * REG, y, x] = torch.cat((onehot(15), onehot(15), onehot(0), onehot(0)))
                    if n % 4 == 3:
                        f[b, 4 * REG :, y, x] = -50.0
                        f[b, 4 * REG + int(gt[b, g, 0]), y, x] = 50.0
                    elif n % 4 == 1:
                        f[b, 4 * REG :, y, x] = -50.0
        a0 += h * w
    return _std("peak", gt, "built", feats=feats)


def _tiny_case():
    """A 0.02-pixel box round the first stride-4 centre (2, 2) of each image with a prediction of 0.004 cells a side (IoU 0.39) and
    nothing else: CIoU's eps terms weigh 4e-3 of the union in grid units and 16 times less in pixels, so this is where a box loss
    computed in pixels shows.  The anchor is the level's first, where 0.5 - d keeps the most bits."""
    gt = _table([[[8, 1.99, 1.99, 2.01, 2.01]], [[1, 1.99, 1.99, 2.01, 2.01]]])
    feats = _rand_heads(88, 2, 10, (64, 64), S4)
    for b in range(2):
        feats[0][b, : 4 * REG, 0, 0] = torch.tensor([0.0, math.log(0.004)] + [-30.0] * 14).repeat(4)
        feats[0][b, 4 * REG :, 0, 0] = -4.0
        feats[0][b, 4 * REG + int(gt[b, 0, 0]), 0, 0] = 3.0
    return _std("tiny", gt, "built", feats=feats)


def _ties_case():
    """Box (4, 4, 28, 28), centre 16: its 36 stride-4 anchors all carry ONE row (every side one-hot at bin 3 with logit 100, so the decoded
    distance is exactly 3 in fp32 and in float64), and mirror images about the centre have bit-equal CIoU.  The metric classes are 4, 8,
    4, ... anchors wide: ranks 5..12 tie exactly across the top-10 boundary and the lowest anchor indices are taken.  The other levels'
    anchors in the box score sigmoid(-50).  Image 1: the same box twice, other class logits, plus a box that shares anchors."""
    gt = _table([[[3, 4.0, 4.0, 28.0, 28.0]], [[3, 4.0, 4.0, 28.0, 28.0], [6, 4.0, 4.0, 28.0, 28.0], [1, 12.0, 12.0, 36.0, 36.0]]])
    feats = _rand_heads(55, 2, 10, (64, 64), S4)
    row = torch.cat((torch.where(torch.arange(REG) == 3, 100.0, 0.0).repeat(4), torch.tensor([-2.0, 0.5, -1.0, 2.0, -3.0, 0.0, 1.5, -0.5, -1.5, 1.0])))
    for b in range(2):
        feats[0][b, :, 1:9, 1:9] = row[:, None, None]
        for f in feats[1:]:
            f[b, 4 * REG :] = -50.0
    return _std("ties", gt, "built", feats=feats)


def build_case(cid):
    tag, _, kind = cid.partition("-")
    if tag == "edge":
        return _std(cid, _table([_edge_rows(0), _edge_rows(1), _edge_rows(-1)]), kind)
    if tag == "sliver":
        return _std(cid, _table([[r for r, _ in SLIVER_ROWS[:6]], [r for r, _ in SLIVER_ROWS[6:]]]), kind)
    if tag == "whole":
        return _std(cid, _table([[[2, 0.0, 0.0, 64.0, 64.0], [4, 70.0, 70.0, 90.0, 90.0], [5, -40.0, -40.0, 20.0, 20.0], [6, 20.0, 24.0, 50.0, 44.0]],
                                 [[1, -10.0, -20.0, 80.0, 90.0], [3, -20.0, 70.0, -5.0, 90.0], [7, 8.5, 30.0, 30.0, 55.5]]]), kind)
    if tag == "dup":
        a, c = [3, 10.0, 10.0, 40.0, 40.0], [[0, 6.0, 8.0, 58.0, 60.0], [1, 14.0, 16.0, 50.0, 52.0], [2, 22.0, 24.0, 42.0, 44.0]]
        return _std(cid, _table([[a, a, [5, 30.5, 33.0, 61.0, 57.0]], [[2] + a[1:], [5] + a[1:]], [[4, 21.0, 5.0, 47.0, 31.0]] + c + [[4, 21.0, 5.0, 47.0, 31.0]]]), kind)
    if tag == "crowd":
        g = torch.Generator().manual_seed(5)
        j = (torch.rand(12, 4, generator=g) * 6 - 3).tolist()
        return _std(cid, _table([[[i % 3, 16 + q[0], 16 + q[1], 40 + q[2], 40 + q[3]] for i, q in enumerate(j)], _rand_boxes(6, 3, 10, (64, 64))]), kind)
    if tag == "pad":
        rows = _rand_boxes(21, 20, 10, (64, 64))
        return _std(cid, _table([[], rows[:7] + [None, None] + rows[7:15] + [None] + rows[15:] + [None]]), kind)
    if tag == "gmax0":
        return _std(cid, torch.zeros(2, 0, 5), kind)
    if tag == "clamp":  # 62-pixel boxes 6 pixels thick hold stride-4 anchors only; the end columns / rows are past 14.99 cells from the far edge
        return _std(cid, _table([[[2, 1.0, 29.0, 63.0, 35.0], [5, 8.0, 40.0, 30.0, 60.0]], [[7, 25.0, 1.0, 31.0, 63.0], [0, 36.0, 10.0, 60.0, 30.0]]]), kind)
    if tag == "rect":
        hw = (64, 96)
        return _std(cid, _table([[[1, 50.0, 6.0, 92.0, 30.0], [3, 66.5, 33.0, 94.0, 61.0], [8, 5.0, 20.0, 40.0, 58.0]], _rand_boxes(31, 4, 10, hw)]), kind, hw=hw)
    if tag in ("nc1", "nc3", "nc80"):
        nc = int(tag[2:])
        return _std(cid, _table([_rand_boxes(41 + nc, 5, nc, (64, 64), classes=[0, nc - 1]), _rand_boxes(42 + nc, 4, nc, (64, 64), classes=[nc - 1, 0])]), kind, nc=nc)
    if tag == "lv3":
        return _std(cid, _table([_rand_boxes(51, 4, 10, (64, 64)), _rand_boxes(52, 3, 10, (64, 64))]), kind, strides=(8.0, 16.0, 32.0))
    if tag in ("k1", "k13"):
        return _std(cid, _table([_rand_boxes(61, 5, 10, (64, 64)), _rand_boxes(62, 6, 10, (64, 64))]), kind, topk=int(tag[1:]), grad=False)
    if tag == "peak":
        return _peak_case()
    if tag == "ties":
        return _ties_case()
    if tag == "tiny":
        return _tiny_case()
    raise KeyError(cid)


CASE_IDS = ["edge-R", "edge-C", "sliver-R", "sliver-C", "whole-R", "whole-C", "dup-R", "dup-C", "crowd-C", "pad-R", "gmax0-R", "clamp-C", "rect-R", "rect-C",
            "nc1-R", "nc3-R", "nc80-R", "lv3-C", "k1-R", "k13-R", "peak", "ties", "tiny"]
C_CASES = [c for c in CASE_IDS if c.endswith("-C")]
PITCH_CASES = [("edge-C", ld) for ld in (74, 76, 80, 88)] + [("nc3-R", ld) for ld in (67, 68, 72, 76, 80, 88)]  # 76 / 80 (nc 10) and 68 (nc 3): whole-row gradient path
