"""Helpers of the tile-fusion tests (not collected): ``fuse_ref``, a numpy restatement of ``dy_tile_fuse`` on top of ``merge_ref``
(tests/_tile_util.py), the hand-built split object that no tile sees whole, and the seeds of the end-to-end frames."""
import numpy as np

from tests._tile_util import F32, merge_ref

MODES = {"union": 1, "wbf": 2}

# block_frame seeds (tests/_tile_util.py) of the 200 x 300 end-to-end frames at tile 128, overlap 0.25, merge threshold 0.6, chosen on the CPU
# oracle so that BOTH hold for the seed: (a) the oracle keeps >= 0.02 from the per-tile NMS threshold and from the merge threshold of the
# run's metric and every anchor's score >= 1e-4 from conf (the condition of tests/test_tile_merge_gpu.py::_expected), and (b) at least one
# kept row has members >= 2 and a fused box that differs from the suppress result.  Seeds that miss either were passed over, nothing was
# loosened.  tests/test_tile_fuse_gpu.py asserts both conditions again before it compares.
FUSE_SEEDS = {("union", "ios"): (4, 7, 13), ("wbf", "iou"): (4, 7, 13)}

# One object [46, 10, 100, 30] on a 64 x 160 frame that neither 64 x 64 tile (at x = 0 and x = 48) sees whole: tile 0 sees [46, 64], tile 1
# sees [48, 100].  IoS = 16 / 18, IoU = 320 / 1080.
SPLIT_OFFS = np.array([[0, 0], [0, 48]], np.int32)
SPLIT_FRAME = (64, 160)


def split_rows():
    rows = np.zeros((2, 4, 6), F32)
    rows[0, 0] = [46, 10, 64, 30, 0.9, 1]
    rows[1, 0] = [0, 10, 52, 30, 0.8, 1]
    return rows, np.array([1, 1], np.int32), SPLIT_OFFS


def fuse_ref(rows, counts, offs, frame_hw, thr, metric, agnostic, merge_max_det, mode):
    """``dy_tile_fuse`` in numpy.  The kept rows are ``merge_ref``'s; a candidate that is not kept goes to the kept row of smallest index that
    stands before it in the sorted list and whose own box suppresses it (fp32, operation by operation as in ``merge_ref``), or is dropped.
    ``mode``: "union" / 1 or "wbf" / 2.  Returns out (F, merge_max_det, 6), count (F), index (F, merge_max_det), members (F, merge_max_det)."""
    mode = MODES.get(mode, mode)
    assert mode in (1, 2), mode
    out, cnt, idx = merge_ref(rows, counts, offs, frame_hw, thr, metric, agnostic, merge_max_det)
    out = out.copy()
    rows, counts, offs = np.asarray(rows, F32), np.asarray(counts, np.int64), np.asarray(offs, np.int64).reshape(-1, 2)
    K, md = len(offs), rows.shape[1]
    F = rows.shape[0] // K
    members = np.zeros((F, merge_max_det), np.int32)
    thr = F32(thr)
    fh, fw = F32(frame_hw[0]), F32(frame_hw[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        for f in range(F):
            nk = int(cnt[f])
            if nk == 0:
                continue
            r, c = rows[f * K : (f + 1) * K], counts[f * K : (f + 1) * K]
            tile, rr = np.nonzero(np.arange(md)[None, :] < c[:, None])  # candidates in slot order
            slot = tile * md + rr
            cand = r[tile, rr]
            box = cand[:, :4] + offs[tile][:, [1, 0, 1, 0]].astype(F32)
            score, cls = cand[:, 4], cand[:, 5].astype(np.int64)
            order = np.argsort(-score, kind="stable")
            pos = np.empty(len(order), np.int64)
            pos[order] = np.arange(len(order))  # place of every candidate in the sorted list
            area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
            kept = np.searchsorted(slot, idx[f, :nk])  # candidate of every kept row (slot is ascending)
            assert np.array_equal(slot[kept], idx[f, :nk])
            kb, ka, kc, kp = box[kept], area[kept], cls[kept], pos[kept]
            owner = np.full(len(slot), -1, np.int64)
            owner[kept] = np.arange(nk)
            rest = np.nonzero(owner < 0)[0]
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
                owner[j] = np.where(sup.any(1), sup.argmax(1), -1)  # the first kept row that matches
            got = owner >= 0
            members[f, :nk] = np.bincount(owner[got], minlength=nk)
            if mode == 1:
                fused = kb.copy()
                for col, fn in ((0, np.minimum), (1, np.minimum), (2, np.maximum), (3, np.maximum)):
                    fn.at(fused[:, col], owner[got], box[got, col])
            else:
                wgt = np.rint(score * F32(65536)).astype(np.int64)
                q = np.rint(box * F32(64)).astype(np.int64)
                S = np.zeros(nk, np.int64)
                X = np.zeros((nk, 4), np.int64)
                np.add.at(S, owner[got], wgt[got])
                np.add.at(X, owner[got], wgt[got, None] * q[got])
                assert np.abs(X).max() < 2**53
                fused = ((X.astype(np.float64) / S.astype(np.float64)[:, None]) * 0.015625).astype(F32)
                own = (members[f, :nk] == 1) | (S == 0)
                fused[own] = kb[own]
            lim = np.array([fw, fh, fw, fh], F32)
            out[f, :nk, :4] = np.minimum(np.maximum(fused, F32(0)), lim[None, :])
    return out, cnt, idx, members
