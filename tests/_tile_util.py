"""Helpers of the tiled-inference tests (not collected): a numpy fp32 restatement of ``dy_tile_merge`` (the oracle of the GPU tests) and a
seeded generator of per-tile detection rows whose overlaps are known by construction."""
import numpy as np

F32 = np.float32

# (F, K, max_det, nc, frame (h, w), tile, overlap): the shapes of tests/test_tile_merge_gpu.py; K is what tile_offsets gives for the frame
CASES = {
    "one_tile": (1, 1, 8, 2, (64, 64), 64, 0.25),
    "lds": (3, 6, 300, 10, (200, 300), 128, 0.25),
    "4k": (2, 40, 300, 10, (512, 800), 128, 0.25),
    "limit": (1, 109, 300, 3, (128, 10496), 128, 0.25),
    "parent6": (1, 6, 300, 10, (200, 300), 128, 0.25),
    "parent40": (1, 40, 300, 10, (512, 800), 128, 0.25),
}
SEEDS = {"one_tile": 1, "lds": 1, "4k": 1, "limit": 1, "parent6": 38, "parent40": 1}  # seeds whose counts hold 0 and max_det and that have cut objects
IOU_THR, IOS_THR, MARGIN = 0.6, 0.8, 0.02  # the thresholds of the GPU tests; no pair may come closer to them than the margin


def tile_offsets(h, w, tile, overlap):
    from drone_yolo_amd.engine.tiling import tile_offsets as f

    return f(h, w, tile, overlap)


def merge_ref(rows, counts, offs, frame_hw, thr, metric, agnostic, merge_max_det):
    """``dy_tile_merge`` in numpy, fp32 operation by operation.  rows (F*K, max_det, 6), counts (F*K), offs (K, 2) = (y, x).
    Returns out (F, merge_max_det, 6), count (F), index (F, merge_max_det) with -1 beyond the count."""
    rows, counts, offs = np.asarray(rows, F32), np.asarray(counts, np.int64), np.asarray(offs, np.int64).reshape(-1, 2)
    K, md = len(offs), rows.shape[1]
    F = rows.shape[0] // K
    out = np.zeros((F, merge_max_det, 6), F32)
    cnt = np.zeros((F,), np.int32)
    idx = np.full((F, merge_max_det), -1, np.int32)
    thr = F32(thr)
    fh, fw = F32(frame_hw[0]), F32(frame_hw[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        for f in range(F):
            r, c = rows[f * K : (f + 1) * K], counts[f * K : (f + 1) * K]
            tile, rr = np.nonzero(np.arange(md)[None, :] < c[:, None])  # candidates in slot order
            slot = tile * md + rr
            cand = r[tile, rr]
            box = cand[:, :4] + offs[tile][:, [1, 0, 1, 0]].astype(F32)  # one fp32 add of an integer-valued float
            score, cls = cand[:, 4], cand[:, 5].astype(np.int64)
            order = np.argsort(-score, kind="stable")  # descending score, ties by ascending slot
            area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
            kb, ka, kc = np.zeros((merge_max_det, 4), F32), np.zeros((merge_max_det,), F32), np.zeros((merge_max_det,), np.int64)
            nk = 0
            for i in order:
                if nk >= merge_max_det:
                    break
                b = box[i]
                w = np.maximum(F32(0), np.minimum(kb[:nk, 2], b[2]) - np.maximum(kb[:nk, 0], b[0]))
                h = np.maximum(F32(0), np.minimum(kb[:nk, 3], b[3]) - np.maximum(kb[:nk, 1], b[1]))
                inter = w * h
                den = np.minimum(ka[:nk], area[i]) if metric else (ka[:nk] + area[i] - inter)
                sup = (inter / den) > thr
                if not agnostic:
                    sup &= kc[:nk] == cls[i]
                if sup.any():
                    continue
                kb[nk], ka[nk], kc[nk] = b, area[i], cls[i]
                out[f, nk] = (min(max(b[0], F32(0)), fw), min(max(b[1], F32(0)), fh), min(max(b[2], F32(0)), fw), min(max(b[3], F32(0)), fh), score[i], F32(cls[i]))
                idx[f, nk] = slot[i]
                nk += 1
            cnt[f] = nk
    return out, cnt, idx


def pair_measures(a, b):
    """float64 (IoU, IoS) of matching rows of two (n, 4) xyxy arrays."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    w = np.clip(np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]), 0, None)
    h = np.clip(np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]), 0, None)
    inter = w * h
    aa, ab = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / np.maximum(aa + ab - inter, 1e-300), inter / np.maximum(np.minimum(aa, ab), 1e-300)


def tile_rows(seed, F, K, max_det, nc, frame_hw, tile, overlap, with_meta=False):
    """Per-tile detection rows of F frames, built by construction (seeded).

    Objects sit in the cells of a lattice, one per cell and strictly inside it, so boxes of different objects never overlap.  Every tile
    that contains an object whole sees it: the object's box with every edge moved by at most 1.5 % of its size (so two views differ by at
    most 3 % per edge and their IoU is above 0.85), shifted to tile coordinates.  An object that a tile would cut is dropped, except for the
    cut objects made on purpose: they straddle the right edge of a tile column with 33-47 % of their width inside; those tiles see the
    clipped part (IoU to the whole box in 0.3-0.5, IoS >= 0.95; their edges move by at most 0.4 %), tiles that hold them whole see the whole box.
    The object density varies in bands across the frame, the rows of a tile are in descending score and cut at max_det, one tile per frame is
    emptied (and of three or more frames the middle one has no rows at all): counts are ragged and include 0 and max_det (where the density allows).  A share of the views repeat their object's score exactly
    and a share of the objects take scores from a grid of 1/64, so there are exact ties inside and across objects.  8 % of the views of the objects that are not cut carry the next class instead of their
    object's: a class-aware merge keeps them beside their duplicates, an agnostic one does not.

    Returns rows (F*K, max_det, 6) fp32, counts (F*K) int32, offs (K, 2) int32; with ``with_meta`` also obj (F*K, max_det) int64 = the
    frame's object of every row (-1 beyond the count), cut: per frame the set of cut objects whose views all survived, and cell (F*K, max_det, 4)
    float64 = the lattice cell of the row's object in frame pixels."""
    rng = np.random.default_rng(seed)
    hf, wf = frame_hw
    offs = np.asarray(tile_offsets(hf, wf, tile, overlap), np.int64)
    assert len(offs) == K, f"{frame_hw} at tile {tile}, overlap {overlap} has {len(offs)} tiles, not {K}"
    pitch = max(4.0, min(16.0, tile / np.sqrt(1.5 * max_det)))  # about 1.5 max_det cells per tile: the dense bands overflow max_det
    ny, nx = int(hf // pitch), int(wf // pitch)
    rows = np.zeros((F * K, max_det, 6), F32)
    counts = np.zeros((F * K,), np.int32)
    obj = np.full((F * K, max_det), -1, np.int64)
    cell = np.zeros((F * K, max_det, 4), np.float64)
    cuts = []
    xedges = sorted({int(x) + tile for _, x in offs if int(x) + tile < wf}) if K > 1 else []  # right edges of tile columns inside the frame
    ox, oy = offs[None, :, 1].astype(np.float64), offs[None, :, 0].astype(np.float64)
    for f in range(F):
        # cut objects: two cells wide (the one that holds the edge and the next), 35-45 % of the width left of the edge
        taken = np.zeros((ny, nx), bool)
        cb, cs, ce, cl = [], [], [], []
        for e in xedges:
            ix = int((e - 0.01) // pitch)
            for iy in range(ny):
                if rng.random() >= 0.9 or ix + 1 >= nx or taken[iy, ix] or taken[iy, ix + 1]:
                    continue
                sz = np.array([rng.uniform(0.5, 0.6), rng.uniform(0.5, 0.8)]) * pitch
                x1 = e - rng.uniform(0.35, 0.45) * sz[0]
                y1 = iy * pitch + 0.05 * pitch + rng.random() * (0.9 * pitch - sz[1])
                if x1 < ix * pitch + 0.02 * pitch:
                    continue
                taken[iy, ix] = taken[iy, ix + 1] = True
                cb.append([x1, y1, x1 + sz[0], y1 + sz[1]]), cs.append(sz), ce.append(e)
                cl.append([ix * pitch, iy * pitch, (ix + 2) * pitch, (iy + 1) * pitch])
        # the other objects: one per cell, kept with a probability that varies in eight bands across the frame
        band = rng.uniform(0.1, 1.0, 8)
        gx = np.arange(nx)[None, :].repeat(ny, 0)
        keep = (rng.random((ny, nx)) < band[np.minimum((8 * gx * pitch / wf).astype(np.int64), 7)]) & ~taken
        iy, ix = np.nonzero(keep)
        n = len(iy)
        sz = rng.uniform(0.5, 0.8, (n, 2)) * pitch
        x1 = ix * pitch + 0.05 * pitch + rng.random(n) * (0.9 * pitch - sz[:, 0])
        y1 = iy * pitch + 0.05 * pitch + rng.random(n) * (0.9 * pitch - sz[:, 1])
        box = np.concatenate([np.stack([x1, y1, x1 + sz[:, 0], y1 + sz[:, 1]], 1), np.asarray(cb, np.float64).reshape(-1, 4)])
        lat = np.concatenate([np.stack([ix * pitch, iy * pitch, (ix + 1) * pitch, (iy + 1) * pitch], 1), np.asarray(cl, np.float64).reshape(-1, 4)])
        sz = np.concatenate([sz, np.asarray(cs, np.float64).reshape(-1, 2)])
        edge = np.concatenate([np.full(n, -1.0), np.asarray(ce, np.float64)])
        jit = np.where(edge >= 0, 0.004, 0.015)
        N = len(box)
        ocls = rng.integers(0, nc, N)
        base = rng.uniform(0.05, 0.99, N)
        base = np.where(rng.random(N) < 0.3, np.round(base * 64) / 64, base).astype(F32)
        # which tile sees which object: whole, clipped at the tile's right edge (cut objects only), or not at all; anything else drops the object
        m = (0.02 * sz.max(1))[:, None]
        b0, b1, b2, b3 = (box[:, j : j + 1] for j in range(4))
        apart = (np.minimum(b2, ox + tile) <= np.maximum(b0, ox) - m) | (np.minimum(b3, oy + tile) <= np.maximum(b1, oy) - m)
        whole = (b0 >= ox + m) & (b1 >= oy + m) & (b2 <= ox + tile - m) & (b3 <= oy + tile - m)
        clipped = (edge[:, None] >= 0) & (ox + tile == edge[:, None]) & (b0 >= ox + m) & (b1 >= oy + m) & (b3 <= oy + tile - m) & ~whole & ~apart
        seen = whole | clipped
        ok = ~(~apart & ~seen).any(1) & seen.any(1) & ((edge < 0) | (whole.any(1) & clipped.any(1)))
        vi, vk = np.nonzero(seen & ok[:, None])
        nv = len(vi)
        v = box[vi] + rng.uniform(-1, 1, (nv, 4)) * (jit[vi, None] * sz[vi][:, [0, 1, 0, 1]]) - offs[vk][:, [1, 0, 1, 0]]
        v = np.clip(v, 0, tile).astype(F32)  # (what the per-tile pass does to its boxes)
        noisy = np.clip(base[vi].astype(np.float64) + rng.uniform(-0.02, 0.02, nv), 0.03, 0.995).astype(F32)
        score = np.where(rng.random(nv) < 0.3, base[vi], noisy).astype(F32)
        vcls = np.where((rng.random(nv) < 0.08) & (edge[vi] < 0), (ocls[vi] + 1) % nc, ocls[vi])  # a share of the views (never a cut object's) names the next class
        n_views = np.bincount(vi, minlength=N)
        empty = int(rng.integers(0, K)) if K > 1 else -1
        live = (vk != empty) & (not (F >= 3 and f == F // 2))  # one tile of every frame sees nothing; of three or more frames the middle one is empty
        vi, vk, v, score, vcls = vi[live], vk[live], v[live], score[live], vcls[live]
        order = np.lexsort((np.arange(len(vi)), -score, vk))  # per tile: descending score, then construction order
        vi, vk, v, score, vcls = vi[order], vk[order], v[order], score[order], vcls[order]
        start = np.searchsorted(vk, np.arange(K))
        rank = np.arange(len(vk)) - start[vk]
        top = rank < max_det
        vi, vk, v, score, rank, vcls = vi[top], vk[top], v[top], score[top], rank[top], vcls[top]
        t = f * K + vk
        rows[t, rank, :4], rows[t, rank, 4], rows[t, rank, 5] = v, score, vcls.astype(F32)
        obj[t, rank], cell[t, rank] = vi, lat[vi]
        counts[f * K : (f + 1) * K] = np.bincount(vk, minlength=K)
        kept_views = np.bincount(vi, minlength=N)
        cuts.append({int(o) for o in np.nonzero((edge >= 0) & ok & (kept_views == n_views))[0]})
    if with_meta:
        return rows, counts, offs.astype(np.int32), obj, cuts, cell
    return rows, counts, offs.astype(np.int32)


def frame_boxes(rows, counts, offs, f, K):
    """The candidates of frame f in frame pixels (float64): boxes (n, 4), cls (n), tile (n), r (n)."""
    md = rows.shape[1]
    c = np.asarray(counts[f * K : (f + 1) * K], np.int64)
    tile, rr = np.nonzero(np.arange(md)[None, :] < c[:, None])
    cand = rows[f * K + tile, rr].astype(np.float64)
    o = np.asarray(offs, np.float64)[tile]
    return cand[:, :4] + o[:, [1, 0, 1, 0]], cand[:, 5].astype(np.int64), tile, rr


def same_class_pair_measures(box, cls):
    """float64 (IoU, IoS) of every pair i < j of one class among (n, 4) boxes (empty arrays when there is none)."""
    i, j = np.triu_indices(len(box), 1)
    same = np.asarray(cls)[i] == np.asarray(cls)[j]
    if not same.any():
        return np.zeros(0), np.zeros(0)
    return pair_measures(np.asarray(box)[i[same]], np.asarray(box)[j[same]])


def oracle_tile_chain(O, d, sd, frame, tile, overlap, nc, conf=0.25, iou=0.7, max_det=300):
    """The per-tile half of the tiled chain on the CPU oracle, as tests/test_model_api_gpu.py::test_tiled_inference_matches_oracle_chain runs it:
    numpy crops (padded with 114 where the frame ends) -> O.forward -> O.non_max_suppression per tile -> clip to the tile.
    Returns rows (K, max_det, 6) fp32, counts (K) int32, offs (K, 2) int32 and margins = (the smallest distance of any anchor's best class
    score from conf, the smallest distance of a same-class IoU among a tile's candidates from iou)."""
    import torch

    hf, wf = frame.shape[:2]
    offs = np.asarray(tile_offsets(hf, wf, tile, overlap), np.int32)
    crops = []
    for y, x in offs:
        c = np.full((tile, tile, 3), 114, np.uint8)
        part = frame[y : y + tile, x : x + tile]
        c[: part.shape[0], : part.shape[1]] = part
        crops.append(torch.from_numpy(np.ascontiguousarray(c[:, :, ::-1].transpose(2, 0, 1))).float() / 255)
    with torch.no_grad():
        yy, _ = O.forward(d, sd, torch.stack(crops))
    det, _ = O.non_max_suppression(yy, conf, iou, max_det=max_det, nc=nc, return_index=True)
    rows, counts = np.zeros((len(offs), max_det, 6), F32), np.zeros((len(offs),), np.int32)
    best, arg = yy[:, 4 : 4 + nc].max(1)
    m_conf, m_iou = float((best - conf).abs().min()), 1.0
    for k, r in enumerate(det):
        r = r.clone()
        r[:, :4] = O.clip_boxes(r[:, :4], (tile, tile))  # each tile is an image of its own to the predictor (detect/predict.py:59-73)
        rows[k, : len(r)], counts[k] = r.numpy(), len(r)
        cand = best[k] > conf
        xywh = yy[k, :4, cand].T.numpy().astype(np.float64)
        box = np.concatenate([xywh[:, :2] - xywh[:, 2:] / 2, xywh[:, :2] + xywh[:, 2:] / 2], 1)
        pi, _ = same_class_pair_measures(box, arg[k, cand].numpy())
        if len(pi):
            m_iou = min(m_iou, float(np.abs(pi - iou).min()))
    return rows, counts, offs, (m_conf, m_iou)


def merge_margin(rows, counts, offs, thr, metric):
    """The smallest distance from thr of a same-class IoU (metric 0) or IoS (metric 1) among the per-tile rows of ONE frame, in frame pixels."""
    box, cls, _, _ = frame_boxes(rows, counts, offs, 0, len(offs))
    m = same_class_pair_measures(box, cls)[metric]
    return float(np.abs(m - thr).min()) if len(m) else 1.0


def block_frame(seed, shape, n=10):
    """A seeded HWC uint8 frame: ten solid rectangles of random colour (10-31 px a side) on the letterbox grey.  The fixture model finds a few
    boxes per tile on such a frame, few enough that seeds exist whose scores and overlaps keep clear of every threshold of the chain."""
    rng = np.random.default_rng(seed)
    f = np.full(tuple(shape) + (3,), 114, np.uint8)
    for _ in range(n):
        h, w = rng.integers(10, 32, 2)
        y, x = rng.integers(0, shape[0] - h), rng.integers(0, shape[1] - w)
        f[y : y + h, x : x + w] = rng.integers(0, 256, 3, dtype=np.uint8)
    return f
