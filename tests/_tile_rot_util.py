"""Helpers of the oriented-box tile-merge tests (not collected): a numpy fp32 restatement of ``dy_tile_merge_rotated`` (the oracle of the GPU
tests), a float64 greedy run that records every ProbIoU it decides on (the margin the inputs must keep from the threshold), a seeded
generator of per-tile rows (x, y, w, h, theta, conf, cls) and the hand-made cases.

The margin rule is tests/test_obb_gpu.py's: M = 8 x max |p32 - p64| over the recorded pairs, and every recorded pair lies at least M from
the threshold.  p32 is the restatement's ProbIoU (numpy's fp32 sin / cos / log / exp, which are not the device's bit for bit), p64
tests/_obb_util.py::probiou64 on the same boxes in float64; a pair that far from the threshold is decided alike by both and by the kernel."""
import functools
import math

import numpy as np

from tests import _obb_util as U

F32 = np.float32
THR = U.IOU  # 0.45: the ProbIoU threshold of every case (chain_boxes is built for it)

# name -> (F, K, max_det, nc, frame (h, w), tile, overlap, fill): K is what tile_offsets gives for the frame; fill = the lowest object density
CASES = {
    "one_tile": (1, 1, 300, 3, (64, 64), 64, 0.25, 0.1),
    "ragged": (3, 6, 300, 10, (200, 300), 128, 0.25, 0.1),
    "chunks": (4, 2, 300, 3, (64, 112), 64, 0.25, 0.9),
    "12k": (1, 40, 300, 10, (512, 800), 128, 0.25, 0.1),
    "limit": (1, 109, 300, 3, (128, 10496), 128, 0.25, 0.1),
}
CHUNK_TOTALS = (63, 64, 65, 129)  # candidates per frame of "chunks": around the scan's chunk of 64
# seeds found on the CPU (tests/test_tile_merge_rotated_host.py asserts what they were chosen for): the margin holds class-aware and agnostic,
# "ragged" has a tile with no rows and one with max_det rows
SEEDS = {"one_tile": 1, "ragged": 1, "chunks": 1, "12k": 1, "limit": 1}
# (case, merge_max_det) of the GPU runs: 16 truncates in the middle of a chunk; at 4096 the kept list pushes the 12,000-slot sort into the workspace
RUNS = [("one_tile", 1000), ("ragged", 1000), ("ragged", 16), ("chunks", 1000), ("12k", 1000), ("12k", 4096), ("limit", 1000)]


def tile_offsets(h, w, tile, overlap):
    from drone_yolo_amd.engine.tiling import tile_offsets as f

    return f(h, w, tile, overlap)


# ---- the kernel's arithmetic in numpy fp32, operation by operation (csrc/probiou.h) ------------------------------------------------------
def cov_rows32(x, y, w, h, th):
    """rnms_row: (x, y, a, b, c) of fp32 arrays."""
    x, y, w, h, th = (np.asarray(v, F32) for v in (x, y, w, h, th))
    a, b = (w * w) / F32(12), (h * h) / F32(12)
    cs, sn = np.cos(th), np.sin(th)
    cs2, sn2 = cs * cs, sn * sn
    return x, y, a * cs2 + b * sn2, a * sn2 + b * cs2, ((a - b) * cs) * sn


def probiou32(r1, r2):
    """rnms_probiou(r1, r2) of two tuples of fp32 arrays (x, y, a, b, c) that broadcast against each other; r1 is the kept row."""
    x1, y1, a1, b1, c1 = r1
    x2, y2, a2, b2, c2 = r2
    eps = F32(1e-7)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sa, sb, sc = a1 + a2, b1 + b2, c1 + c2
        dy, dx = y1 - y2, x1 - x2
        det = sa * sb - sc * sc
        den = det + eps
        t1 = ((sa * (dy * dy) + sb * (dx * dx)) / den) * F32(0.25)
        t2 = (((sc * (x2 - x1)) * dy) / den) * F32(0.5)
        d1, d2 = a1 * b1 - c1 * c1, a2 * b2 - c2 * c2
        d1, d2 = np.where(d1 < 0, F32(0), d1), np.where(d2 < 0, F32(0), d2)
        t3 = np.log(det / (F32(4) * np.sqrt(d1 * d2) + eps) + eps) * F32(0.5)
        bd = (t1 + t2) + t3
        bd = np.where(bd < eps, eps, np.where(bd > F32(100), F32(100), bd))  # (a NaN stays a NaN, as the kernel's ternaries leave it)
        hd = np.sqrt((F32(1) - np.exp(-bd)) + eps)
        return (F32(1) - hd).astype(F32)


def far_bound(thr):
    """csrc/tile_merge.hip::tmr_far_bound: the value of t1 + t2 above which the kernel does not finish the expression (with det > 0)."""
    if not thr >= 1e-3:
        return math.inf
    return float(F32(-math.log(1.0 - (1.0 - float(F32(thr))) ** 2 + 1e-7) + 9.0))


def distance_terms32(r1, r2):
    """(t1 + t2, det) as probiou32 computes them."""
    x1, y1, a1, b1, c1 = r1
    x2, y2, a2, b2, c2 = r2
    eps = F32(1e-7)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sa, sb, sc = a1 + a2, b1 + b2, c1 + c2
        dy, dx = y1 - y2, x1 - x2
        det = sa * sb - sc * sc
        den = det + eps
        return ((sa * (dy * dy) + sb * (dx * dx)) / den) * F32(0.25) + (((sc * (x2 - x1)) * dy) / den) * F32(0.5), det


def probiou64_rows(one, many):
    """tests/_obb_util.py::probiou64's expression for ONE xywhr box against (k, 5) boxes, float64: probiou64(concatenate((one, many)))[0, 1:]
    without the k x k pairs nobody asks for (the host test holds the two to each other)."""
    def cov(b):
        a_, b_ = b[..., 2] ** 2 / 12, b[..., 3] ** 2 / 12
        cos, sin = np.cos(b[..., 4]), np.sin(b[..., 4])
        return a_ * cos**2 + b_ * sin**2, a_ * sin**2 + b_ * cos**2, (a_ - b_) * cos * sin

    one, many = np.asarray(one, np.float64), np.asarray(many, np.float64)
    (a1, b1, c1), (a2, b2, c2) = cov(one), cov(many)
    sa, sb, sc = a1 + a2, b1 + b2, c1 + c2
    dx, dy = one[0] - many[:, 0], one[1] - many[:, 1]
    eps = 1e-7
    det = sa * sb - sc**2
    t1 = (sa * dy**2 + sb * dx**2) / (det + eps) * 0.25
    t2 = (sc * (-dx) * dy) / (det + eps) * 0.5
    d1, d2 = np.clip(a1 * b1 - c1**2, 0, None), np.clip(a2 * b2 - c2**2, 0, None)
    with np.errstate(invalid="ignore"):
        t3 = np.log(det / (4 * np.sqrt(d1 * d2) + eps) + eps) * 0.5
    bd = np.clip(t1 + t2 + t3, eps, 100.0)
    return 1 - np.sqrt(1.0 - np.exp(-bd) + eps)


def _candidates(rows, counts, offs, f, K):
    """The candidates of frame f in slot order: slot, tile, row-in-tile, the (n, 7) rows."""
    md = rows.shape[1]
    c = np.clip(np.asarray(counts[f * K : (f + 1) * K], np.int64), 0, md)
    tile, rr = np.nonzero(np.arange(md)[None, :] < c[:, None])
    return tile * md + rr, tile, rows[f * K + tile, rr]


def merge_ref_rotated(rows, counts, offs, frame_hw, thr, agnostic, merge_max_det):
    """``dy_tile_merge_rotated`` in numpy.  rows (F*K, max_det, 7), counts (F*K), offs (K, 2) = (y, x).  Returns out (F, merge_max_det, 7),
    count (F), index (F, merge_max_det) with -1 beyond the count."""
    rows, offs = np.asarray(rows, F32), np.asarray(offs, np.int64).reshape(-1, 2)
    K = len(offs)
    F = rows.shape[0] // K
    out = np.zeros((F, merge_max_det, 7), F32)
    cnt = np.zeros((F,), np.int32)
    idx = np.full((F, merge_max_det), -1, np.int32)
    thr = F32(thr)
    fh, fw = F32(frame_hw[0]), F32(frame_hw[1])
    for f in range(F):
        slot, tile, cand = _candidates(rows, counts, offs, f, K)
        x = cand[:, 0] + offs[tile, 1].astype(F32)  # one fp32 add of an integer-valued float
        y = cand[:, 1] + offs[tile, 0].astype(F32)
        w, h, th, score, cls = cand[:, 2], cand[:, 3], cand[:, 4], cand[:, 5], cand[:, 6].astype(np.int64)
        cov = np.stack(cov_rows32(x, y, w, h, th), 1)  # once per candidate
        order = np.argsort(-score, kind="stable")  # descending conf, ties by ascending slot
        kr, kc = np.zeros((merge_max_det, 5), F32), np.zeros((merge_max_det,), np.int64)
        nk = 0
        for i in order:
            if nk >= merge_max_det:
                break
            sup = probiou32(tuple(kr[:nk, j] for j in range(5)), tuple(cov[i, j] for j in range(5))) >= thr  # a NaN does not suppress
            if not agnostic:
                sup &= kc[:nk] == cls[i]
            if sup.any():
                continue
            kr[nk], kc[nk] = cov[i], cls[i]
            out[f, nk] = (min(max(x[i], F32(0)), fw), min(max(y[i], F32(0)), fh), min(max(w[i], F32(0)), fw), min(max(h[i], F32(0)), fh), th[i], score[i], F32(cls[i]))
            idx[f, nk] = slot[i]
            nk += 1
        cnt[f] = nk
    return out, cnt, idx


def greedy64(rows, counts, offs, thr, agnostic, merge_max_det):
    """The same greedy merge decided in float64 (probiou64's expression on the frame-coordinate boxes).  Returns per frame the kept slots, and over all
    frames the float64 and the fp32 ProbIoU of every (kept-so-far, candidate) pair it evaluated among rows the class rule lets meet."""
    rows, offs = np.asarray(rows, F32), np.asarray(offs, np.int64).reshape(-1, 2)
    K = len(offs)
    kept_slots, p64s, p32s = [], [np.zeros(0)], [np.zeros(0, F32)]
    for f in range(rows.shape[0] // K):
        slot, tile, cand = _candidates(rows, counts, offs, f, K)
        box = cand[:, :5].astype(np.float64)
        box[:, 0] += offs[tile, 1]
        box[:, 1] += offs[tile, 0]
        cov = np.stack(cov_rows32(cand[:, 0] + offs[tile, 1].astype(F32), cand[:, 1] + offs[tile, 0].astype(F32), cand[:, 2], cand[:, 3], cand[:, 4]), 1)
        cls = cand[:, 6].astype(np.int64)
        order = np.argsort(-cand[:, 5], kind="stable")
        kept = []
        for i in order:
            if len(kept) >= merge_max_det:
                break
            k = np.asarray(kept, np.int64)
            if not agnostic:
                k = k[cls[k] == cls[i]]
            if len(k):
                p64 = probiou64_rows(box[i], box[k])
                p64s.append(p64)
                p32s.append(probiou32(tuple(cov[k, j] for j in range(5)), tuple(cov[i, j] for j in range(5))))
                if (p64 >= thr).any():
                    continue
            kept.append(i)
        kept_slots.append(slot[np.asarray(kept, np.int64)])
    return kept_slots, np.concatenate(p64s), np.concatenate(p32s)


def margin(p64, p32, thr):
    """(M, the smallest distance of a recorded pair from thr): the inputs keep the rule when the second is at least the first."""
    if len(p64) == 0:
        return 0.0, 1.0
    assert np.isfinite(p64).all() and np.isfinite(p32).all(), "a recorded pair has no finite ProbIoU"
    return 8.0 * float(np.abs(p32.astype(np.float64) - p64).max()), float(np.abs(p64 - thr).min())


# ---- generated rows ------------------------------------------------------------------------------------------------------------------------
def rot_tile_rows(seed, F, K, max_det, nc, frame_hw, tile, overlap, fill=0.1, hole=True):
    """Per-tile oriented rows of F frames, built by construction (seeded).

    Objects sit in the cells of a lattice (pitch p), one per cell with its circumscribed circle inside the cell: sides in [0.2, 0.55] p, angle in
    [0, pi / 2) as dy_scale_rboxes leaves it, so two objects are at least a box apart (ProbIoU below 0.1) .  Every tile that holds an object's
    circle sees it: centre moved by at most 1 % of the sides, sides scaled by at most 1 %, angle turned by at most 0.01 rad (ProbIoU to
    another view above 0.9), shifted to tile coordinates -- so most candidates are cross-tile duplicates.  8 % of the views name the next class.
    All scores of a frame are distinct (a view's score lies near its object's).  The object density varies in eight bands across the frame
    (at least ``fill``); the rows of a tile are in descending score, cut at max_det; one tile of every frame (K > 1) sees nothing and of
    three or more frames the middle one has no rows (``hole``).  Returns rows (F*K, max_det, 7) fp32, counts (F*K) int32, offs (K, 2) int32 = (y, x)."""
    rng = np.random.default_rng(seed)
    hf, wf = frame_hw
    offs = np.asarray(tile_offsets(hf, wf, tile, overlap), np.int64)
    assert len(offs) == K, f"{frame_hw} at tile {tile}, overlap {overlap} has {len(offs)} tiles, not {K}"
    pitch = max(4.0, min(16.0, tile / np.sqrt(2.2 * max_det)))  # about 2.2 max_det cells per tile: the dense bands overflow max_det
    ny, nx = int(hf // pitch), int(wf // pitch)
    rows = np.zeros((F * K, max_det, 7), F32)
    counts = np.zeros((F * K,), np.int32)
    oy, ox = offs[None, :, 0].astype(np.float64), offs[None, :, 1].astype(np.float64)
    for f in range(F):
        band = rng.uniform(fill, 1.0, 8)
        gx = np.arange(nx)[None, :].repeat(ny, 0)
        iy, ix = np.nonzero(rng.random((ny, nx)) < band[np.minimum((8 * gx * pitch / wf).astype(np.int64), 7)])
        n = len(iy)
        wh = rng.uniform(0.2, 0.55, (n, 2)) * pitch
        rad = 0.5 * np.hypot(wh[:, 0], wh[:, 1])
        room = (0.48 * pitch - rad)[:, None]
        cxy = (np.stack([ix, iy], 1) + 0.5) * pitch + rng.uniform(-1, 1, (n, 2)) * room
        th = rng.uniform(0.0, 0.5 * math.pi, n)
        ocls = rng.integers(0, nc, n)
        base = rng.uniform(0.05, 0.99, n)
        r = (rad + 0.02 * pitch)[:, None]
        seen = (cxy[:, :1] - r >= ox) & (cxy[:, :1] + r <= ox + tile) & (cxy[:, 1:] - r >= oy) & (cxy[:, 1:] + r <= oy + tile)
        vi, vk = np.nonzero(seen)
        nv = len(vi)
        vxy = cxy[vi] + rng.uniform(-1, 1, (nv, 2)) * 0.01 * wh[vi] - offs[vk][:, [1, 0]]
        vwh = wh[vi] * (1 + rng.uniform(-1, 1, (nv, 2)) * 0.01)
        vth = th[vi] + rng.uniform(-1, 1, nv) * 0.01
        raw = base[vi] + rng.uniform(-0.02, 0.02, nv)
        score = np.zeros(nv, F32)
        score[np.argsort(raw, kind="stable")] = np.linspace(0.05, 0.99, nv).astype(F32)  # distinct, in the order of the noisy scores
        assert len(np.unique(score)) == nv
        vcls = np.where(rng.random(nv) < 0.08, (ocls[vi] + 1) % nc, ocls[vi])
        empty = int(rng.integers(0, K)) if K > 1 and hole else -1
        live = (vk != empty) & (not (hole and F >= 3 and f == F // 2))
        vk, vxy, vwh, vth, score, vcls = vk[live], vxy[live], vwh[live], vth[live], score[live], vcls[live]
        order = np.lexsort((-score, vk))
        vk, vxy, vwh, vth, score, vcls = vk[order], vxy[order], vwh[order], vth[order], score[order], vcls[order]
        rank = np.arange(len(vk)) - np.searchsorted(vk, np.arange(K))[vk]
        top = rank < max_det
        t = f * K + vk[top]
        rows[t, rank[top]] = np.concatenate([vxy[top], vwh[top], vth[top, None], score[top, None], vcls[top, None]], 1).astype(F32)
        counts[f * K : (f + 1) * K] = np.bincount(vk[top], minlength=K)
    return rows, counts, offs.astype(np.int32)


@functools.lru_cache(maxsize=None)
def case_rows(name):
    """(rows, counts, offs) of a generated case (shared, not modified).  "chunks": the counts are cut down so that its four frames have 63,
    64, 65 and 129 candidates (the rows behind a count stay in the buffer: the kernel must not read them)."""
    F, K, md, nc, hw, tile, overlap, fill = CASES[name]
    rows, counts, offs = rot_tile_rows(SEEDS[name], F, K, md, nc, hw, tile, overlap, fill, hole=name != "chunks")
    if name == "chunks":
        for f, total in enumerate(CHUNK_TOTALS):
            c = counts[f * K : (f + 1) * K]
            assert c.sum() >= total, f"chunks: frame {f} has {c.sum()} candidates, fewer than {total}"
            c[0] = min(c[0], total // 2)
            c[1] = total - c[0]
            assert 0 <= c[1] <= md and c.sum() == total
    for a in (rows, counts, offs):
        a.setflags(write=False)
    return rows, counts, offs


@functools.lru_cache(maxsize=None)
def case_ref(name, agnostic, keep):
    rows, counts, offs = case_rows(name)
    return merge_ref_rotated(rows, counts, offs, CASES[name][4], THR, agnostic, keep)


# ---- hand-made cases -----------------------------------------------------------------------------------------------------------------------
HAND_FRAME = (256, 320)
HAND_OFFS = np.asarray([(0, 0), (0, 96), (64, 32), (128, 192)], np.int32)  # (y, x): x and y differ in every tile but the first
HAND_MAX_DET = 8


def place(views, frame_hw=HAND_FRAME, offs=HAND_OFFS, max_det=HAND_MAX_DET):
    """views: (tile, (x, y, w, h, theta) in FRAME pixels, score, cls) in the order the tile lists them -> rows, counts, offs."""
    rows = np.zeros((len(offs), max_det, 7), F32)
    counts = np.zeros((len(offs),), np.int32)
    for tile, box, score, cls in views:
        r = counts[tile]
        rows[tile, r] = (box[0] - offs[tile][1], box[1] - offs[tile][0], box[2], box[3], box[4], score, cls)
        counts[tile] += 1
    return rows, counts, np.asarray(offs, np.int32)


def hand_case(name):
    """-> rows, counts, offs, {agnostic: the slots the merge must keep, in order}.  Slot = tile * HAND_MAX_DET + row."""
    md = HAND_MAX_DET
    if name == "chain":  # A suppresses B; B alone overlaps C: greedy keeps A and C, the reference's fast NMS only A
        a, b, c = U.chain_boxes(U.CHAIN_D)
        return (*place([(0, a, 0.9, 1), (1, b, 0.8, 1), (2, c, 0.7, 1)]), {False: [0, 2 * md], True: [0, 2 * md]})
    if name == "same_place":  # one box seen twice under two classes
        box = (150.0, 100.0, 40.0, 16.0, 0.7)
        return (*place([(1, box, 0.9, 0), (2, box, 0.8, 1)]), {False: [md, 2 * md], True: [md]})
    if name == "offsets":  # one object seen from tiles 1 (x 96, y 0) and 2 (x 32, y 64): with ox and oy swapped the views land 150 px apart
        return (*place([(1, (150.0, 100.0, 40.0, 16.0, 0.4), 0.9, 0), (2, (150.5, 100.25, 40.0, 16.0, 0.4), 0.8, 0)]), {False: [md], True: [md]})
    if name == "clamp":  # a centre right of the frame, one above it, a width and a height larger than the frame
        views = [(3, (326.0, 200.0, 20.0, 10.0, 0.2), 0.9, 0), (0, (50.0, -3.0, 20.0, 10.0, 0.2), 0.8, 1), (2, (160.0, 128.0, 400.0, 300.0, 0.0), 0.7, 2)]
        return (*place(views), {False: [3 * md, 0, 2 * md], True: [3 * md, 0, 2 * md]})
    if name == "degenerate":  # zero width and zero height, each alone in its class (class-aware only: their ProbIoU is not decided with a margin)
        views = [(0, (60.0, 60.0, 0.0, 12.0, 0.3), 0.9, 0), (1, (200.0, 60.0, 14.0, 0.0, 0.3), 0.8, 1), (2, (100.0, 150.0, 30.0, 12.0, 0.3), 0.7, 2)]
        return (*place(views), {False: [0, md, 2 * md]})
    raise KeyError(name)


HAND_CASES = ("chain", "same_place", "offsets", "clamp", "degenerate")
