"""Helpers of the tiled-segmentation tests (not collected): ``owner_ref``, a numpy fp32 restatement of ``dy_tile_mask_owner`` on top of
``merge_ref`` (tests/_tile_util.py); ``frame_masks_ref``, the float64 reference of ``dy_tile_process_mask`` (value v and magnitude S per
pixel and member, as ``_mask_util.blend64`` does it for ``dy_process_mask``); and the seeded cases both test files share."""
from functools import lru_cache

import numpy as np

from tests._fuse_util import SPLIT_FRAME, SPLIT_OFFS
from tests._mask_util import NM, UNSURE, degenerate_boxes, make_boxes
from tests._tile_util import F32, merge_ref, tile_offsets

TILE, GRID = 64, 16
STRIDES = (1, 2, 4)


def owner_ref(rows, counts, offs, frame_hw, thr, metric, agnostic, merge_max_det, stitch):
    """``dy_tile_mask_owner`` in numpy: owner (F, K * max_det) int32 and ``merge_ref``'s (out, count, index).  The kept rows are
    ``merge_ref``'s; with ``stitch`` a candidate that is not kept goes to the kept row of smallest index that stands before it in the sorted
    list and whose own box suppresses it (``fuse_ref``'s rule, fp32 operation by operation)."""
    out, cnt, idx = merge_ref(rows, counts, offs, frame_hw, thr, metric, agnostic, merge_max_det)
    rows, counts, offs = np.asarray(rows, F32), np.asarray(counts, np.int64), np.asarray(offs, np.int64).reshape(-1, 2)
    K, md = len(offs), rows.shape[1]
    F = rows.shape[0] // K
    owner = np.full((F, K * md), -1, np.int32)
    thr = F32(thr)
    with np.errstate(divide="ignore", invalid="ignore"):
        for f in range(F):
            nk = int(cnt[f])
            owner[f, idx[f, :nk]] = np.arange(nk)
            if nk == 0 or not stitch:
                continue
            r, c = rows[f * K : (f + 1) * K], counts[f * K : (f + 1) * K]
            tile, rr = np.nonzero(np.arange(md)[None, :] < c[:, None])
            slot = tile * md + rr
            cand = r[tile, rr]
            box = cand[:, :4] + offs[tile][:, [1, 0, 1, 0]].astype(F32)
            score, cls = cand[:, 4], cand[:, 5].astype(np.int64)
            order = np.argsort(-score, kind="stable")
            pos = np.empty(len(order), np.int64)
            pos[order] = np.arange(len(order))
            area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
            kept = np.searchsorted(slot, idx[f, :nk])
            kb, ka, kc, kp = box[kept], area[kept], cls[kept], pos[kept]
            rest = np.nonzero(owner[f, slot] < 0)[0]
            for lo in range(0, len(rest), 256):
                j = rest[lo : lo + 256]
                b = box[j]
                w = np.maximum(F32(0), np.minimum(kb[None, :, 2], b[:, None, 2]) - np.maximum(kb[None, :, 0], b[:, None, 0]))
                h = np.maximum(F32(0), np.minimum(kb[None, :, 3], b[:, None, 3]) - np.maximum(kb[None, :, 1], b[:, None, 1]))
                inter = w * h
                den = np.minimum(ka[None, :], area[j][:, None]) if metric else (ka[None, :] + area[j][:, None] - inter)
                sup = ((inter / den) > thr) & (kp[None, :] < pos[j][:, None])
                if not agnostic:
                    sup &= kc[None, :] == cls[j][:, None]
                owner[f, slot[j]] = np.where(sup.any(1), sup.argmax(1), -1)
    return owner, (out, cnt, idx)


def owner_histogram(owner, merge_max_det):
    """members (F, merge_max_det): how many slots every kept row owns."""
    return np.stack([np.bincount(o[o >= 0], minlength=merge_max_det) for o in owner]).astype(np.int32)


def _axis(n_out, s, o, tile, g):
    """Per output coordinate: inside the tile, i0, i1, l0, l1 (float64 restatement of the kernel's source coordinates)."""
    t = (np.arange(n_out) + 0.5) * s - o
    inside = (t >= 0) & (t < tile)
    src = np.maximum(0.25 * t - 0.5, 0.0)
    i0 = np.clip(np.floor(src).astype(np.int64), 0, g - 1)
    i1 = np.minimum(i0 + 1, g - 1)
    l1 = src - i0
    return inside, i0, i1, 1.0 - l1, l1, t


def frame_masks_ref(protos, side, counts, offs, owner, dest, total, tile, frame_hw, s):
    """protos (F*K, mh, mw, 32), side (F*K, max_det, 36), counts (F*K), offs (K, 2), owner (F, K*max_det), dest (F, M) -> (ref, unsure, inbox),
    bool (total, oh, ow).  ref = OR over the members of v > 0; unsure: a member has |v| < UNSURE * S there and no other member is surely set;
    inbox: the pixel's centre lies in a member's box (the denominator of the unsure share)."""
    protos, side = np.asarray(protos, np.float64), np.asarray(side, np.float32)
    offs = np.asarray(offs, np.int64).reshape(-1, 2)
    K, md = len(offs), side.shape[1]
    F = protos.shape[0] // K
    mh, mw = protos.shape[1:3]
    oh, ow = -(-frame_hw[0] // s), -(-frame_hw[1] // s)
    ref, sure, weak, inbox = (np.zeros((total, oh, ow), bool) for _ in range(4))
    with np.errstate(invalid="ignore"):
        for f in range(F):
            for j in np.nonzero(owner[f] >= 0)[0]:
                k, r = divmod(int(j), md)
                b = f * K + k
                m = int(dest[f, owner[f, j]])
                if r >= counts[b] or m < 0:
                    continue
                oy, ox = offs[k]
                iny, y0, y1, ly0, ly1, ty = _axis(oh, s, oy, tile, mh)
                inx, x0, x1, lx0, lx1, tx = _axis(ow, s, ox, tile, mw)
                box = side[b, r, :4]
                c = side[b, r, 4:].astype(np.float64)
                q = (box * F32(0.25)).astype(np.float64)
                xs, ys = np.arange(mw)[None, :], np.arange(mh)[:, None]
                keep = (xs >= q[0]) & (xs < q[2]) & (ys >= q[1]) & (ys < q[3])
                val = (protos[b] @ c) * keep
                mag = (np.abs(protos[b]) @ np.abs(c)) * keep

                def mix(a):
                    top = a[y0][:, x0] * lx0 + a[y0][:, x1] * lx1
                    bot = a[y1][:, x0] * lx0 + a[y1][:, x1] * lx1
                    return top * ly0[:, None] + bot * ly1[:, None]

                inside = iny[:, None] & inx[None, :]
                v, S = mix(val) * inside, mix(mag) * inside
                w = np.abs(v) < UNSURE * S
                ref[m] |= v > 0
                sure[m] |= (v > 0) & ~w
                weak[m] |= w
                bq = box.astype(np.float64)
                inbox[m] |= inside & ((tx >= bq[0]) & (tx < bq[2]))[None, :] & ((ty >= bq[1]) & (ty < bq[3]))[:, None]
    return ref, weak & ~sure, inbox


# ---- the cases: tile 64, proto 16 x 16 ---------------------------------------------------------------------------------------------
# name -> (frames, frame (h, w), offsets or None (tile_offsets at overlap 0.25), max_det, seed)
CASES = {
    "one_tile": (2, (64, 64), None, 8, 3100),
    "split": (2, SPLIT_FRAME, SPLIT_OFFS, 8, 3200),
    "six": (8, (100, 150), None, 32, 3300),  # K = 6, x offset 86: no multiple of 4
    "small": (2, (40, 50), None, 8, 3400),  # smaller than the tile
    "three": (1, (100, 150), None, 8, 3500),  # hand-written: one row with three members in three tiles
}


def case_inputs(name):
    """A case's inputs, regenerated from its seed (numpy): protos (F*K, 16, 16, 32) and coefficients N(0, 1); boxes in tile pixels, sides
    0.3-0.9 of the tile, no crop edge within 1e-2 of a proto column / row; counts that include 0 and max_det; rows beyond the counts NaN.
    Every case's first tile ends with a NaN-corner box and one narrower than a proto pixel.  owner: the valid slots in a seeded order,
    grouped into kept rows of one to three members (every other row has one); dest: a seeded permutation of the rows with every fifth row left out (-1)."""
    import torch

    F, frame_hw, offs, md, seed = CASES[name]
    offs = np.asarray(tile_offsets(frame_hw[0], frame_hw[1], TILE, 0.25) if offs is None else offs, np.int32).reshape(-1, 2)
    K = len(offs)
    rng = np.random.default_rng(seed)
    protos = torch.randn(F * K, GRID, GRID, NM, generator=torch.Generator().manual_seed(seed)).numpy()
    coef = torch.randn(F * K, md, NM, generator=torch.Generator().manual_seed(seed + 1)).numpy()
    counts = rng.integers(md // 2, md + 1, F * K).astype(np.int32)
    counts[0] = md
    if F * K > 1:
        counts[-1] = 0
    side = np.full((F * K, md, 4 + NM), np.nan, np.float32)
    for b in range(F * K):
        n = int(counts[b])
        side[b, :n, :4] = make_boxes(rng, n, TILE, TILE, (0.25, 0.25))
        side[b, :n, 4:] = coef[b, :n]
    side[0, md - 2 : md, :4] = degenerate_boxes(TILE, TILE, (0.25, 0.25))[5:7]
    M = 64 if name != "six" else 256
    owner = np.full((F, K * md), -1, np.int32)
    dest = np.full((F, M), -1, np.int32)
    total = 0
    for f in range(F):
        tile, rr = np.nonzero(np.arange(md)[None, :] < counts[f * K : (f + 1) * K, None])
        slots = rng.permutation(tile * md + rr)
        if name == "three":  # kept row 0: the first rows of tiles 0, 1, 2, one box that reaches into all of them
            for k in range(3):
                side[k, 0, :4] = np.array([2.3, 2.7, 61.4, 61.6], np.float32)
            slots = np.concatenate([[0, md, 2 * md], [v for v in slots if v not in (0, md, 2 * md)]])
        t, i = 0, 0
        while i < len(slots) and t < M:
            g = 3 if name == "three" and t == 0 else (1 if t % 2 else int(rng.integers(1, 4)))  # every other row has one member
            owner[f, slots[i : i + g]] = t
            i, t = i + g, t + 1
        emit = np.array([v for v in range(t) if v % 5 != 4], np.int64)
        dest[f, emit] = total + rng.permutation(len(emit))
        total += len(emit)
    return dict(protos=protos, side=side, counts=counts, offs=offs, owner=owner, dest=dest, total=total, frame_hw=tuple(frame_hw), F=F, K=K, max_det=md, M=M)


@lru_cache(maxsize=None)
def case_reference(name, s):
    """(inputs, (ref, unsure, inbox)) of a case at stride s, computed once per process; callers leave the arrays unchanged."""
    inp = case_inputs(name)
    out = frame_masks_ref(inp["protos"], inp["side"], inp["counts"], inp["offs"], inp["owner"], inp["dest"], inp["total"], TILE, inp["frame_hw"], s)
    for a in out:
        a.setflags(write=False)
    return inp, out
