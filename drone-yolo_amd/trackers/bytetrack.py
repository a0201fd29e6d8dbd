"""ByteTrack on the padded NMS output (reference: ultralytics/trackers/byte_tracker.py ``BYTETracker.update`` / ``STrack``,
trackers/utils/kalman_filter.py ``KalmanFilterXYAH``, trackers/utils/matching.py, trackers/basetrack.py, cfg/trackers/bytetrack.yaml).

Two classes with one constructor and one surface (``update`` / ``update_batch`` / ``reset``):

* ``ByteTracker``: the host path, numpy in float64 — what ``device_track=False`` selects and what makes the logic checkable on a CPU.
* ``DeviceByteTracker``: the ``dy_track_step`` kernel (csrc/track.hip); state, outputs and counts stay on the device.

The tracks of a stream are a struct of arrays over ``max_tracks`` slots (tracked, lost and unconfirmed together), not a list of objects.
What the reference's three Python lists hold follows from the slot fields:

    tracked_stracks   state == TRACKED (``activated`` tells confirmed from unconfirmed)
    lost_stracks      state == LOST or state == REMOVED   (a slot is freed the moment it leaves this list)
    removed_stracks   only membership by id matters: the slot's ``in_removed`` flag

Quirks of the reference that are behaviour: a lost track that times out is marked REMOVED but stays in the lost list for one
more update (the list is filtered against ``removed_stracks`` before this frame's removals are appended) and can be re-found in it; a
track re-found that way carries its id in ``removed_stracks`` for good, so it leaves at once when it is lost again; an image without
detections never reaches the tracker; detection boxes go xyxy -> xywh -> tlwh -> xyah in float32; ``initiate`` leaves a float32 mean
(and float32 products in the standard deviations) until the first predict / update.  Rows come out in ascending track id.

``rotated=True`` (both classes): the tracker of an oriented-box model (trackers/track.py:69-88 ``is_obb``).  Rows in are (n, 7)
[x, y, w, h, r, conf, cls], rows out (k, 9) [x, y, w, h, r, id, score, cls, idx].  The Kalman filter is the same one on (x, y, aspect, h);
centre and size come straight from the row (no xyxy -> xywh step); every cost is ``1 - batch_probiou`` on xywha rows rounded to float32
(``STrack.xywha``: the corner from the mean, then the centre back from the corner), with ``fuse_score`` on top; the angle is not filtered:
a track holds the angle of the detection it last matched, a lost track a stale one.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np

FREE, TRACKED, LOST, REMOVED = 0, 1, 2, 3
CFG_KEYS = ("tracker_type", "track_high_thresh", "track_low_thresh", "new_track_thresh", "track_buffer", "match_thresh", "fuse_score")
_CFG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfg", "trackers")
_F32 = np.float32


def load_tracker_cfg(tracker="bytetrack.yaml") -> SimpleNamespace:
    """A tracker YAML (a path, or a name under cfg/trackers), a dict or a namespace -> namespace with the reference's seven keys."""
    if isinstance(tracker, SimpleNamespace):
        cfg = vars(tracker)
    elif isinstance(tracker, dict):
        cfg = tracker
    else:
        import yaml

        path = str(tracker)
        if not os.path.isfile(path):
            path = os.path.join(_CFG_DIR, os.path.basename(path))
        if not os.path.isfile(path):
            raise FileNotFoundError(f"tracker settings '{tracker}' not found (looked in {_CFG_DIR} too)")
        with open(path) as f:
            cfg = yaml.safe_load(f)
    kind = cfg.get("tracker_type", "bytetrack")
    if kind == "botsort":
        raise NotImplementedError("tracker_type 'botsort' is not built: its camera-motion compensation needs cv2 and its ReID branch a second network; use bytetrack.yaml")
    if kind != "bytetrack":
        raise AssertionError(f"Only 'bytetrack' is supported, but got '{kind}'")
    missing = [k for k in CFG_KEYS if k not in cfg]
    if missing:
        raise KeyError(f"tracker settings lack {missing}")
    return SimpleNamespace(**{k: cfg[k] for k in CFG_KEYS})


def detections_f32(rows: np.ndarray):
    """(n, 6) rows [x1, y1, x2, y2, conf, cls] -> (xyxy, xyah, conf, cls) as the reference's ``STrack`` holds a detection: ``Boxes.xywh`` in
    float32, the corner ``x - w / 2`` in float64 (the index column makes the array float64) rounded to float32, everything after in float32."""
    b = np.ascontiguousarray(rows[:, :4], dtype=_F32)
    xywh = np.empty_like(b)
    xywh[:, 0] = (b[:, 0] + b[:, 2]) / 2
    xywh[:, 1] = (b[:, 1] + b[:, 3]) / 2
    xywh[:, 2] = b[:, 2] - b[:, 0]
    xywh[:, 3] = b[:, 3] - b[:, 1]
    w64 = xywh.astype(np.float64)
    tlwh = xywh.copy()
    tlwh[:, :2] = (w64[:, :2] - w64[:, 2:] / 2).astype(_F32)
    xyxy = tlwh.copy()
    xyxy[:, 2:] += xyxy[:, :2]
    xyah = tlwh.copy()
    xyah[:, :2] += xyah[:, 2:] / 2
    with np.errstate(all="ignore"):
        xyah[:, 2] /= xyah[:, 3]
    return xyxy, xyah, np.asarray(rows[:, 4], dtype=_F32), np.asarray(rows[:, 5], dtype=_F32)


def detections_r32(rows: np.ndarray):
    """(n, 7) rows [x, y, w, h, r, conf, cls] -> (xywha, xyah, conf, cls) as the reference's ``STrack`` holds an oriented detection
    (byte_tracker.py:68-79): centre and size from the row, the corner ``x - w / 2`` in float64 rounded to float32, ``xywha`` = that corner
    plus half the size in float32 with the row's angle."""
    xywh = np.ascontiguousarray(rows[:, :4], dtype=_F32)
    w64 = xywh.astype(np.float64)
    tlwh = xywh.copy()
    tlwh[:, :2] = (w64[:, :2] - w64[:, 2:] / 2).astype(_F32)
    xyah = tlwh.copy()
    xyah[:, :2] += xyah[:, 2:] / 2
    xywha = np.concatenate([xyah[:, :2], tlwh[:, 2:], np.asarray(rows[:, 4:5], dtype=_F32)], axis=1)
    with np.errstate(all="ignore"):
        xyah[:, 2] /= xyah[:, 3]
    return xywha, xyah, np.asarray(rows[:, 5], dtype=_F32), np.asarray(rows[:, 6], dtype=_F32)


def probiou_cost(a: np.ndarray, b: np.ndarray, scores: Optional[np.ndarray] = None) -> np.ndarray:
    """``1 - batch_probiou(a, b)`` on float32 xywha rows (matching.py:85-101; torch on the CPU as there), then ``fuse_score`` when ``scores``
    is given."""
    from ..utils.metrics import batch_probiou

    a, b = np.ascontiguousarray(a, dtype=_F32).reshape(-1, 5), np.ascontiguousarray(b, dtype=_F32).reshape(-1, 5)
    if not len(a) or not len(b):
        return np.zeros((len(a), len(b)), dtype=_F32)
    with np.errstate(all="ignore"):
        cost = _F32(1) - batch_probiou(a, b).numpy()
        if scores is not None:
            cost = _F32(1) - (_F32(1) - cost) * scores.astype(_F32)[None, :]
    return cost


def iou_cost(a: np.ndarray, b: np.ndarray, scores: Optional[np.ndarray] = None) -> np.ndarray:
    """``1 - bbox_ioa(a, b, iou=True)`` in float32 in its order of operations (eps 1e-7), then ``fuse_score`` when ``scores`` is given."""
    a, b = a.astype(_F32, copy=False), b.astype(_F32, copy=False)
    with np.errstate(all="ignore"):
        iw = (np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])).clip(0)
        ih = (np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])).clip(0)
        inter = iw * ih
        area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :] + ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] - inter
        cost = _F32(1) - inter / (area + _F32(1e-7))
        if scores is not None:
            cost = _F32(1) - (_F32(1) - cost) * scores.astype(_F32)[None, :]
    return cost


def assign(cost: np.ndarray, thresh: float) -> np.ndarray:
    """``matching.linear_assignment(cost, thresh)`` = lapjv(extend_cost=True, cost_limit=thresh): the matching that minimises the sum of
    (cost - thresh) over matched pairs; a pair at or above the limit (or NaN) is no edge.  Solved exactly with scipy on the thresholded
    rectangular problem (one zero column per row stands for 'unmatched').  Returns the column of every row, -1 = unmatched."""
    n, m = cost.shape
    match = np.full(n, -1, dtype=np.int64)
    if n == 0 or m == 0:
        return match
    edge = cost < thresh
    if not edge.any():
        return match
    from scipy.optimize import linear_sum_assignment

    w = np.zeros((n, m + n), dtype=np.float64)
    w[:, :m] = np.where(edge, cost.astype(np.float64) - thresh, 0.0)
    r, c = linear_sum_assignment(w)
    ok = c < m
    ok[ok] = edge[r[ok], c[ok]]
    match[r[ok]] = c[ok]
    return match


def _width_message(shape, width: int, rotated: bool) -> str:
    kind = "a rotated tracker takes [x, y, w, h, r, conf, cls]" if rotated else "a plain tracker takes [x1, y1, x2, y2, conf, cls] (rotated=True for oriented rows)"
    return f"rows of shape {tuple(shape)}: {kind}, {width} columns"


def _rows_of(rows, width: int, rotated: bool) -> np.ndarray:
    """The rows of one image as an (n, width) float32 array; another width is refused (an empty array of any shape is no rows)."""
    rows = np.asarray(rows.detach().cpu() if hasattr(rows, "detach") else rows, dtype=_F32)
    if rows.size == 0:
        return rows.reshape(0, width)
    if rows.ndim == 1 and rows.size == width:  # one row
        return rows.reshape(1, width)
    if rows.ndim != 2 or rows.shape[1] != width:
        raise ValueError(_width_message(rows.shape, width, rotated))
    return rows


class _Stream:
    """The slots of one video stream."""

    def __init__(self, max_tracks: int):
        t = max_tracks
        self.mean = np.zeros((t, 8))
        self.cov = np.zeros((t, 8, 8))
        self.state = np.zeros(t, dtype=np.int32)
        self.activated = np.zeros(t, dtype=bool)
        self.m32 = np.zeros(t, dtype=bool)  # the mean is still initiate's float32 one
        self.in_removed = np.zeros(t, dtype=bool)
        self.id = np.zeros(t, dtype=np.int64)
        self.score = np.zeros(t, dtype=_F32)
        self.cls = np.zeros(t, dtype=_F32)
        self.angle = np.zeros(t, dtype=_F32)  # rotated trackers: the angle of the detection last matched
        self.idx = np.zeros(t, dtype=np.int64)
        self.frame_id = np.zeros(t, dtype=np.int64)
        self.start_frame = np.zeros(t, dtype=np.int64)
        self.tracklet_len = np.zeros(t, dtype=np.int64)
        self.frame = 0
        self.next_id = 0
        self.overflow = 0


class ByteTracker:
    """Host ByteTrack.  ``cfg``: a tracker YAML name / path, dict or namespace; ``streams``: independent video streams of a batch (image k
    of a batch is stream ``k % streams`` at time step ``k // streams``); ``max_tracks``: slots per stream — when they are full no new
    track starts and the stream's ``overflow`` counter goes up; ``rotated``: oriented rows (module docstring)."""

    def __init__(self, cfg="bytetrack.yaml", frame_rate: int = 30, max_tracks: int = 512, streams: int = 1, max_det: int = 300, device=None,
                 rotated: bool = False):
        self.cfg = load_tracker_cfg(cfg)
        self.max_tracks, self.streams, self.max_det = int(max_tracks), int(streams), int(max_det)
        self.rotated = bool(rotated)
        self.row_in, self.row_out = (7, 9) if self.rotated else (6, 8)
        if self.max_tracks < 1 or self.streams < 1:
            raise ValueError("max_tracks and streams must be positive")
        self.max_time_lost = int(frame_rate / 30.0 * self.cfg.track_buffer)
        self.reset()

    def reset(self) -> None:
        self._s = [_Stream(self.max_tracks) for _ in range(self.streams)]
        self.min_margin = float("inf")  # smallest distance of a cost / score from the threshold it was compared with (ties excepted for scores)

    @property
    def overflow(self) -> np.ndarray:
        return np.array([s.overflow for s in self._s], dtype=np.int64)

    @property
    def frame_count(self) -> np.ndarray:
        return np.array([s.frame for s in self._s], dtype=np.int64)

    # ---- pieces ----------------------------------------------------------------------------------------
    def _margin(self, values: np.ndarray, thresh: float, exact_ok: bool = False) -> None:
        v = np.asarray(values, dtype=np.float64).ravel()
        v = np.abs(v[np.isfinite(v)] - float(thresh))
        if exact_ok:
            v = v[v > 0]
        if v.size:
            self.min_margin = min(self.min_margin, float(v.min()))

    @staticmethod
    def _xyxy(st: _Stream, slots: np.ndarray) -> np.ndarray:
        """``STrack.xyxy`` of the slots, rounded to float32 as ``iou_distance`` and ``result`` round it (float32 arithmetic while the mean is
        initiate's float32 one)."""
        m = st.mean[slots, :4]
        out = np.empty((len(slots), 4), dtype=_F32)
        for sel, dt in ((st.m32[slots], _F32), (~st.m32[slots], np.float64)):
            if sel.any():
                r = m[sel].astype(dt)
                r[:, 2] *= r[:, 3]
                r[:, :2] -= r[:, 2:] / 2
                r[:, 2:] += r[:, :2]
                out[sel] = r.astype(_F32)
        return out

    @staticmethod
    def _xywh(st: _Stream, slots: np.ndarray) -> np.ndarray:
        """``STrack.xywh`` of the slots rounded to float32: ``tlwh`` from the mean, then the centre back from the corner, in that order."""
        m = st.mean[slots, :4]
        out = np.empty((len(slots), 4), dtype=_F32)
        for sel, dt in ((st.m32[slots], _F32), (~st.m32[slots], np.float64)):
            if sel.any():
                r = m[sel].astype(dt)
                r[:, 2] *= r[:, 3]
                r[:, :2] -= r[:, 2:] / 2
                r[:, :2] += r[:, 2:] / 2
                out[sel] = r.astype(_F32)
        return out

    def _boxes(self, st: _Stream, slots: np.ndarray) -> np.ndarray:
        """What ``iou_distance`` and ``result`` read of the slots: ``xyxy``, or ``xywha`` of a rotated tracker."""
        if not self.rotated:
            return self._xyxy(st, slots)
        return np.concatenate([self._xywh(st, slots), st.angle[slots, None]], axis=1)

    def _cost(self, a: np.ndarray, b: np.ndarray, scores: Optional[np.ndarray] = None) -> np.ndarray:
        return probiou_cost(a, b, scores) if self.rotated else iou_cost(a, b, scores)

    @staticmethod
    def _predict(st: _Stream, slots: np.ndarray) -> None:
        if not len(slots):
            return
        mean, cov = st.mean[slots], st.cov[slots]
        mean[st.state[slots] != TRACKED, 7] = 0
        h = mean[:, 3]
        sp, sv = (1.0 / 20) * h, (1.0 / 160) * h
        q = np.square(np.stack([sp, sp, 1e-2 * np.ones_like(h), sp, sv, sv, 1e-5 * np.ones_like(h), sv], axis=1))
        mean[:, :4] = mean[:, :4] + mean[:, 4:]
        fp = cov.copy()  # F P: rows 0..3 gain rows 4..7
        fp[:, :4, :] = cov[:, :4, :] + cov[:, 4:, :]
        new = fp.copy()  # (F P) F^T: columns 0..3 gain columns 4..7
        new[:, :, :4] = fp[:, :, :4] + fp[:, :, 4:]
        new[:, np.arange(8), np.arange(8)] += q
        st.mean[slots], st.cov[slots], st.m32[slots] = mean, new, False

    @staticmethod
    def _kalman_update(st: _Stream, slots: np.ndarray, z: np.ndarray) -> None:
        """``KalmanFilterXYAH.update`` of the slots with the float32 measurements ``z`` (n, 4)."""
        if not len(slots):
            return
        mean, cov, m32 = st.mean[slots], st.cov[slots], st.m32[slots]
        h = mean[:, 3]
        s = np.where(m32, (_F32(1.0 / 20) * h.astype(_F32)).astype(np.float64), (1.0 / 20) * h)
        r = np.square(np.stack([s, s, 1e-1 * np.ones_like(h), s], axis=1))
        pc = cov[:, :4, :4].copy()
        pc[:, np.arange(4), np.arange(4)] += r
        kt = np.linalg.solve(pc, cov[:, :4, :])  # K^T = S^-1 (P H^T)^T, (n, 4, 8)
        innov = z.astype(np.float64) - mean[:, :4]
        st.mean[slots] = mean + np.einsum("ni,nij->nj", innov, kt)
        st.cov[slots] = cov - np.einsum("nia,nij,njb->nab", kt, pc, kt)
        st.m32[slots] = False

    def _matched(self, st: _Stream, slots: np.ndarray, det: np.ndarray, xyah, conf, cls, angle=None) -> None:
        """``STrack.update`` (tracked) / ``re_activate`` (lost) of the slots with their detections."""
        if not len(slots):
            return
        self._kalman_update(st, slots, xyah[det])
        was = st.state[slots] == TRACKED
        st.tracklet_len[slots] = np.where(was, st.tracklet_len[slots] + 1, 0)
        st.state[slots], st.activated[slots], st.frame_id[slots] = TRACKED, True, st.frame
        st.score[slots], st.cls[slots], st.idx[slots] = conf[det], cls[det], det
        if angle is not None:
            st.angle[slots] = angle[det]

    # ---- one image of one stream -------------------------------------------------------------------------
    def _step(self, st: _Stream, rows: np.ndarray) -> np.ndarray:
        c = self.cfg
        if len(rows) == 0:  # track.py:79-80: such an image never reaches the tracker
            return np.zeros((0, self.row_out), dtype=_F32)
        st.frame += 1
        dxyxy, dxyah, conf, cls = detections_r32(rows) if self.rotated else detections_f32(rows)  # (dxyxy: xywha rows of a rotated tracker)
        ang = dxyxy[:, 4] if self.rotated else None
        high, low, newt = _F32(c.track_high_thresh), _F32(c.track_low_thresh), _F32(c.new_track_thresh)
        for t in (high, low, newt):
            self._margin(conf, t, exact_ok=True)
        hi = np.nonzero(conf >= high)[0]
        lo = np.nonzero((conf > low) & (conf < high))[0]

        alive = st.state != FREE
        unconf = np.nonzero(alive & (st.state == TRACKED) & ~st.activated)[0]
        pool = np.nonzero(alive & (((st.state == TRACKED) & st.activated) | (st.state == LOST) | (st.state == REMOVED)))[0]
        was_lost = pool[st.state[pool] != TRACKED]
        self._predict(st, pool)

        # first association: the pool against the high-score detections
        cost = self._cost(self._boxes(st, pool), dxyxy[hi], conf[hi] if c.fuse_score else None)
        self._margin(cost, c.match_thresh)
        m = assign(cost, c.match_thresh)
        self._matched(st, pool[m >= 0], hi[m[m >= 0]], dxyah, conf, cls, ang)
        det_free = np.ones(len(hi), dtype=bool)
        det_free[m[m >= 0]] = False
        # second association: what is left of the TRACKED pool against the low-score detections
        rest = pool[m < 0]
        rest = rest[st.state[rest] == TRACKED]
        cost = self._cost(self._boxes(st, rest), dxyxy[lo])
        self._margin(cost, 0.5)
        m2 = assign(cost, 0.5)
        self._matched(st, rest[m2 >= 0], lo[m2[m2 >= 0]], dxyah, conf, cls, ang)
        st.state[rest[m2 < 0]] = LOST
        # unconfirmed tracks against the high-score detections still free
        hi2 = hi[det_free]
        cost = self._cost(self._boxes(st, unconf), dxyxy[hi2], conf[hi2] if c.fuse_score else None)
        self._margin(cost, 0.7)
        m3 = assign(cost, 0.7)
        self._matched(st, unconf[m3 >= 0], hi2[m3[m3 >= 0]], dxyah, conf, cls, ang)
        st.state[unconf[m3 < 0]] = FREE  # removed, and in no list
        # new tracks, ids in ascending detection index
        free3 = np.ones(len(hi2), dtype=bool)
        free3[m3[m3 >= 0]] = False
        new = hi2[free3]
        new = new[~(conf[new] < newt)]
        slots = np.nonzero(st.state == FREE)[0]
        if len(new) > len(slots):
            st.overflow += len(new) - len(slots)
            new = new[: len(slots)]
        slots = slots[: len(new)]
        if len(new):
            h32 = dxyah[new, 3]
            sp, sv = (_F32(2 * (1.0 / 20)) * h32).astype(np.float64), (_F32(10 * (1.0 / 160)) * h32).astype(np.float64)
            one = np.ones(len(new))
            st.mean[slots] = np.concatenate([dxyah[new].astype(np.float64), np.zeros((len(new), 4))], axis=1)
            st.cov[slots] = 0
            st.cov[slots[:, None], np.arange(8), np.arange(8)] = np.square(np.stack([sp, sp, 1e-2 * one, sp, sv, sv, 1e-5 * one, sv], axis=1))
            st.m32[slots], st.in_removed[slots] = True, False
            st.state[slots], st.activated[slots] = TRACKED, st.frame == 1
            st.id[slots] = st.next_id + 1 + np.arange(len(new))
            st.next_id += len(new)
            st.score[slots], st.cls[slots], st.idx[slots] = conf[new], cls[new], new
            if self.rotated:
                st.angle[slots] = ang[new]
            st.frame_id[slots] = st.start_frame[slots] = st.frame
            st.tracklet_len[slots] = 0
        # time-outs of what was in the lost list when the update began; the list is filtered against the removals of EARLIER updates only
        out_of_time = was_lost[(st.state[was_lost] != TRACKED) & (st.frame - st.frame_id[was_lost] > self.max_time_lost)]
        st.state[out_of_time] = REMOVED
        gone = ((st.state == LOST) | (st.state == REMOVED)) & st.in_removed
        st.state[gone] = FREE
        st.in_removed[out_of_time] = True  # (appended after the filter: these stay for one more update)
        # duplicates between the tracked and the lost list: the younger one goes
        ta, tb = np.nonzero(st.state == TRACKED)[0], np.nonzero((st.state == LOST) | (st.state == REMOVED))[0]
        if len(ta) and len(tb):
            pd = self._cost(self._boxes(st, ta), self._boxes(st, tb))
            self._margin(pd, 0.15)
            p, q = np.nonzero(pd < 0.15)
            older_a = (st.frame_id[ta[p]] - st.start_frame[ta[p]]) > (st.frame_id[tb[q]] - st.start_frame[tb[q]])
            st.state[tb[q[older_a]]] = FREE
            st.state[ta[p[~older_a]]] = FREE
        # STrack.result of the activated tracked tracks, in ascending id
        o = np.nonzero((st.state == TRACKED) & st.activated)[0]
        o = o[np.argsort(st.id[o], kind="stable")]
        res = np.empty((len(o), self.row_out), dtype=_F32)
        res[:, : self.row_out - 4] = self._boxes(st, o)
        res[:, -4], res[:, -3], res[:, -2], res[:, -1] = st.id[o], st.score[o], st.cls[o], st.idx[o]
        return res

    # ---- surface -----------------------------------------------------------------------------------------
    def update(self, rows, stream: int = 0) -> np.ndarray:
        """One image of one stream: (n, 6) rows -> (k, 8) float32 [x1, y1, x2, y2, id, score, cls, idx] (``STrack.result``), ascending id;
        a rotated tracker: (n, 7) rows -> (k, 9) [x, y, w, h, r, id, score, cls, idx]."""
        return self._step(self._s[stream], _rows_of(rows, self.row_in, self.rotated))

    def update_batch(self, rows, counts) -> Tuple[np.ndarray, np.ndarray]:
        """A batch of padded rows (F * S, max_det, 6) with counts (F * S,) -> padded (F * S, max_tracks, 8) float32 and counts (int32); a
        rotated tracker: (F * S, max_det, 7) -> (F * S, max_tracks, 9)."""
        rows = np.asarray(rows.detach().cpu() if hasattr(rows, "detach") else rows, dtype=_F32)
        if rows.ndim != 3 or rows.shape[2] != self.row_in:
            raise ValueError(_width_message(rows.shape, self.row_in, self.rotated))
        counts = np.asarray(counts.detach().cpu() if hasattr(counts, "detach") else counts).astype(np.int64)
        if len(rows) % self.streams:
            raise ValueError(f"{len(rows)} images are no multiple of track_streams = {self.streams}")
        out = np.zeros((len(rows), self.max_tracks, self.row_out), dtype=_F32)
        n = np.zeros(len(rows), dtype=np.int32)
        for k in range(len(rows)):
            r = self._step(self._s[k % self.streams], rows[k, : max(0, min(int(counts[k]), rows.shape[1]))])
            out[k, : len(r)], n[k] = r, len(r)
        return out, n


class DeviceByteTracker:
    """ByteTrack in one kernel launch per batch (``dy_track_step``): one workgroup per stream walks its time steps in order; the Kalman
    state lives in device memory between calls.  Same constructor and surface as ``ByteTracker``; ``update_batch`` takes the NMS buffers'
    device tensors and returns device tensors without synchronising."""

    def __init__(self, cfg="bytetrack.yaml", frame_rate: int = 30, max_tracks: int = 512, streams: int = 1, max_det: int = 300, device="cuda",
                 rotated: bool = False):
        import torch

        from .. import hip_ops as H

        self.cfg = load_tracker_cfg(cfg)
        self.max_tracks, self.streams, self.max_det = int(max_tracks), int(streams), int(max_det)
        self.max_time_lost = int(frame_rate / 30.0 * self.cfg.track_buffer)
        self.device = torch.device(device)
        self._H = H
        self.rotated = bool(rotated)
        self.row_in, self.row_out = (7, 9) if self.rotated else (6, 8)
        self.bufs = H.TrackBuffers(self.streams, self.max_tracks, self.max_det, self.device, rotated=self.rotated)
        self.reset()

    def reset(self) -> None:
        self._H.track_reset(self.bufs)

    @property
    def overflow(self) -> np.ndarray:
        return self._H.track_counters(self.bufs)[:, 2].astype(np.int64)

    @property
    def frame_count(self) -> np.ndarray:
        return self._H.track_counters(self.bufs)[:, 0].astype(np.int64)

    def update_batch(self, rows, counts):
        """Device tensors rows (F * S, max_det, 6) fp32 / counts (F * S,) int32 -> (out (F * S, max_tracks, 8), count (F * S,)), views of
        this tracker's output buffers (overwritten by the next call); no host synchronisation.  A rotated tracker: rows (.., 7), out (.., 9)."""
        import torch

        rows = torch.as_tensor(rows, dtype=torch.float32, device=self.device).contiguous()
        counts = torch.as_tensor(counts, device=self.device).to(torch.int32).contiguous()
        if rows.dim() != 3 or rows.shape[2] != self.row_in or rows.shape[1] != self.max_det:
            raise ValueError(f"rows must be (images, max_det = {self.max_det}, {self.row_in}); " + _width_message(rows.shape, self.row_in, self.rotated))
        n = rows.shape[0]
        if n % self.streams:
            raise ValueError(f"{n} images are no multiple of track_streams = {self.streams}")
        return self._H.track_step(self.bufs, (rows, counts), n // self.streams, self.streams, self.cfg, max_time_lost=self.max_time_lost)

    def update(self, rows, stream: int = 0) -> np.ndarray:
        """One image of a single-stream tracker (synchronises; for tests and small uses)."""
        import torch

        if self.streams != 1 or stream != 0:
            raise ValueError("update() serves a single-stream tracker; use update_batch")
        r = torch.as_tensor(_rows_of(rows, self.row_in, self.rotated))
        if len(r) > self.max_det:
            raise ValueError(f"{len(r)} rows exceed max_det = {self.max_det}")
        pad = torch.zeros((1, self.max_det, self.row_in), dtype=torch.float32)
        pad[0, : len(r)] = r
        out, cnt = self.update_batch(pad.to(self.device), torch.tensor([len(r)], dtype=torch.int32, device=self.device))
        k = int(cnt[0])
        return out[0, :k].cpu().numpy()
