"""Writes tests/golden/track_obb.npz: what the REAL reference's ``BYTETracker`` returns on synthetic sequences of ORIENTED detections
(trackers/track.py:69-88 ``is_obb``), for tests/test_track_obb_host.py and tests/test_track_obb_gpu.py.

    python tools/make_track_obb_golden.py

Built on tools/make_track_golden.py: the reference through oracle/make_golden.py::import_reference, the stand-in ``lap`` in ``sys.modules``
before anything under ``ultralytics.trackers`` is imported, every sequence recorded twice with two exact formulations of the assignment
(outputs asserted identical), outputs stored sorted by id, arrays / seeds / settings only.  The tracker is fed an object exposing ``xywhr``,
``conf`` and ``cls`` as the reference's ``OBB`` does; it returns ``STrack.result`` = xywha + [id, score, cls, idx], nine columns.

Sequences: the analogues of the five axis-aligned ones (sparse, crowd, flicker with track_buffer 4, thresholds, gaps) and ``turning``: pairs
of elongated boxes (aspect 4.5..8) crossed over one centre, every pair turning a few degrees per frame through the ``regularize_rboxes``
wrap (the angle stays in [0, pi / 2), width and height swap).  The hulls of a pair coincide while their ProbIoU is about 0.2, so a tracker
that compares hulls cannot tell the two apart.

Per sequence the tool checks, in this order, and takes the next seed when a check fails (nothing is loosened):
  1. the IoU-on-hull answer (xywhr2xyxyxyxy -> min / max -> this repository's axis-aligned host tracker) is computed; on ``turning`` it must
     give another id than the reference's ProbIoU rows to at least one detection;
  2. the margin M = 8 * max |cost32 - cost64| over every pair the sequence evaluates whose float64 ProbIoU lies in [0.1, 0.97] (cost32:
     what the reference's ``iou_distance`` returned, cost64: the same expression in float64 on the same float32 rows), never below 1e-5;
  3. no cost lies within M of the threshold it is compared with (match_thresh, 0.5, 0.7, 0.15);
  4. no score lies within 1e-6 of a score threshold unless it equals it;
  5. the sequence run again with ``batch_probiou`` evaluated in float64 returns the same ids and idx on every frame (near-tied optima
     would part here: a device's cosf / logf / expf differ from the CPU's in the last bits);
plus the two formulations' agreement and the events a sequence is there for.  M, the seeds and the settings go into the file.
"""
from __future__ import annotations

import math
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import make_track_golden as G  # noqa: E402  (install_lap, the two formulations, the defaults)

NAMES = ["sparse", "crowd", "flicker", "thresholds", "gaps", "turning"]
IMG = G.IMG
M_FLOOR = 1e-5


def probiou64(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(n, 5) x (m, 5) xywhr -> (n, m) ProbIoU in float64: batch_probiou's expression (utils/metrics.py:244-275)."""
    a, b = np.asarray(a, np.float64).reshape(-1, 5), np.asarray(b, np.float64).reshape(-1, 5)

    def cov(r):
        p, q = r[:, 2] ** 2 / 12, r[:, 3] ** 2 / 12
        c, s = np.cos(r[:, 4]), np.sin(r[:, 4])
        return p * c**2 + q * s**2, p * s**2 + q * c**2, (p - q) * c * s

    a1, b1, c1 = (t[:, None] for t in cov(a))
    a2, b2, c2 = (t[None, :] for t in cov(b))
    x1, y1, x2, y2 = a[:, 0:1], a[:, 1:2], b[None, :, 0], b[None, :, 1]
    eps = 1e-7
    with np.errstate(all="ignore"):
        det = (a1 + a2) * (b1 + b2) - (c1 + c2) ** 2
        t1 = ((a1 + a2) * (y1 - y2) ** 2 + (b1 + b2) * (x1 - x2) ** 2) / (det + eps) * 0.25
        t2 = ((c1 + c2) * (x2 - x1) * (y1 - y2)) / (det + eps) * 0.5
        t3 = np.log(det / (4 * np.sqrt(np.clip(a1 * b1 - c1**2, 0, None) * np.clip(a2 * b2 - c2**2, 0, None)) + eps) + eps) * 0.5
        bd = np.clip(t1 + t2 + t3, eps, 100.0)
        return 1 - np.sqrt(1.0 - np.exp(-bd) + eps)


def regularize(rows: np.ndarray) -> np.ndarray:
    """ops.regularize_rboxes on the first five columns: the angle into [0, pi / 2), width and height swapped where it was in [pi / 2, pi)."""
    rows = rows.copy()
    t = rows[:, 4]
    swap = t % math.pi >= math.pi / 2
    w, h = rows[:, 2].copy(), rows[:, 3].copy()
    rows[:, 2], rows[:, 3] = np.where(swap, h, w), np.where(swap, w, h)
    rows[:, 4] = t % (math.pi / 2)
    return rows


def hull_rows(rows: np.ndarray) -> np.ndarray:
    """(n, 7) xywhr rows -> (n, 6) [x1, y1, x2, y2, conf, cls]: the axis-aligned hull of the four corners (ops.xywhr2xyxyxyxy -> min / max)."""
    x, y, w, h, t = (rows[:, k].astype(np.float64) for k in range(5))
    c, s = np.cos(t), np.sin(t)
    ex, ey = np.abs(w / 2 * c) + np.abs(h / 2 * s), np.abs(w / 2 * s) + np.abs(h / 2 * c)
    return np.stack([x - ex, y - ey, x + ex, y + ey, rows[:, 5], rows[:, 6]], axis=1).astype(np.float32)


# ---- synthetic scenes ------------------------------------------------------------------------------------
def scene(rng, n_obj, frames, area, long_side, aspect, speed, jitter, omega=0.03, p_visible=0.9, n_cls=2, lanes=0, vanish=None, scores=(0.05, 0.98), pairs=False):
    """Constant-velocity, constant-turn-rate oriented boxes + jitter.  Per frame an (n, 7) float32 array [x, y, w, h, r, conf, cls], regularised
    as the OBB predictor leaves it, in descending score.  ``pairs``: objects 2k and 2k + 1 share centre, velocity and turn rate and stand at
    right angles to one another (an X)."""
    x0, y0, x1, y1 = area
    c = np.stack([rng.uniform(x0, x1, n_obj), rng.uniform(y0, y1, n_obj)], axis=1)
    v = rng.uniform(-speed, speed, (n_obj, 2))
    length = rng.uniform(long_side[0], long_side[1], n_obj)
    wh = np.stack([length, length / rng.uniform(aspect[0], aspect[1], n_obj)], axis=1)
    th = rng.uniform(0, math.pi, n_obj)
    om = rng.uniform(-omega, omega, n_obj)
    if lanes:  # same size and heading, small speed differences: objects overtake one another along a few lines
        c[:, 1] = y0 + (y1 - y0) * (rng.integers(0, lanes, n_obj) + 0.5) / lanes
        v[:, 1] = 0
        v[:, 0] = speed + rng.uniform(-2.0, 2.0, n_obj)
        wh[:] = wh[0]
        th[:] = rng.uniform(-0.1, 0.1, n_obj)
        om[:] = rng.uniform(-0.01, 0.01, n_obj)
    if pairs:
        for k in range(1, n_obj, 2):
            c[k], v[k], om[k] = c[k - 1] + rng.uniform(-1, 1, 2), v[k - 1], om[k - 1]
            th[k] = th[k - 1] + math.pi / 2 + rng.uniform(-0.1, 0.1)
            wh[k] = wh[k - 1] * rng.uniform(0.97, 1.03)
    cls = rng.integers(0, n_cls, n_obj)
    hidden = np.zeros(n_obj, dtype=np.int64)
    out = []
    for f in range(frames):
        rows = []
        for k in range(n_obj):
            p = c[k] + v[k] * f
            if vanish is not None:
                if hidden[k] > 0:
                    hidden[k] -= 1
                    continue
                if f > 2 and rng.random() < vanish:
                    hidden[k] = rng.integers(1, 9)
                    continue
            elif rng.random() > p_visible:
                continue
            j = rng.normal(0, jitter, 5)
            w, h = wh[k] * (1 + 0.02 * j[2:4])
            x, y = p[0] + j[0], p[1] + j[1]
            if not (0 < x < IMG[1] and 0 < y < IMG[0]) or min(w, h) < 2:
                continue
            s = rng.uniform(*scores) if rng.random() < 0.3 else rng.uniform(0.5, 0.98)
            rows.append([x, y, w, h, th[k] + om[k] * f + 0.01 * j[4], s, cls[k]])
        rows = regularize(np.asarray(rows, dtype=np.float64).reshape(-1, 7)).astype(np.float32)
        out.append(rows[np.argsort(-rows[:, 5], kind="stable")])  # as the NMS leaves them
    return out


def make(name, seed):
    rng = np.random.default_rng(seed)
    cfg = dict(G.DEFAULTS)
    if name == "sparse":
        fr = scene(rng, 12, 30, (100, 100, 1100, 600), (40, 110), (1.0, 5.0), 6, 0.8, p_visible=0.9, n_cls=3)
    elif name == "crowd":
        fr = scene(rng, 130, 10, (480, 240, 800, 480), (40, 90), (1.0, 4.0), 3, 0.8, p_visible=0.95, n_cls=2)
    elif name == "flicker":
        cfg["track_buffer"] = 4
        fr = scene(rng, 30, 36, (40, 200, 500, 520), (60, 60), (2.0, 2.0), 9, 0.3, n_cls=1, lanes=3, vanish=0.12, scores=(0.26, 0.98))
    elif name == "thresholds":
        fr = scene(rng, 14, 16, (100, 100, 1100, 600), (40, 110), (1.0, 5.0), 5, 0.8, p_visible=0.95, n_cls=2)
        special = [np.float32(0.25), np.float32(0.1), np.float32(0.25), np.float32(0.1), np.float32(0.2499), np.float32(0.1001)]
        for f, rows in enumerate(fr):
            if f == 9:  # a frame where every score is low
                rows[:, 5] = rng.uniform(0.11, 0.24, len(rows)).astype(np.float32)
            for k in range(min(len(rows), 4)):
                rows[(3 * k + f) % len(rows), 5] = special[(f + k) % len(special)]
    elif name == "gaps":
        fr = scene(rng, 10, 24, (100, 100, 1100, 600), (40, 110), (1.0, 5.0), 6, 0.8, p_visible=0.92, n_cls=2)
        for f in (0, 5, 6, 13, 23):
            fr[f] = np.zeros((0, 7), dtype=np.float32)
    elif name == "turning":
        fr = scene(rng, 12, 30, (150, 150, 1100, 560), (70, 130), (4.5, 8.0), 3, 0.6, omega=0.07, p_visible=0.97, n_cls=1, scores=(0.3, 0.98), pairs=True)
    else:
        raise KeyError(name)
    return fr, cfg


# ---- recording ---------------------------------------------------------------------------------------------
class Probe:
    def __init__(self):
        self.err = 0.0  # max |cost32 - cost64| over the pairs with float64 ProbIoU in [0.1, 0.97]
        self.pairs = 0
        self.dist = []  # |cost - threshold| of every comparison (fused costs for the associations)
        self.score_margin = float("inf")
        self.refound = self.dups = self.second = 0


def run_reference(frames, cfg, probe=None, float64=False):
    import torch
    from ultralytics.trackers import byte_tracker as bt
    from ultralytics.trackers.utils import matching
    from ultralytics.utils import IterableSimpleNamespace

    orig = (matching.linear_assignment, bt.BYTETracker.remove_duplicate_stracks, bt.STrack.re_activate, matching.iou_distance, matching.batch_probiou)

    def la(cost, thresh, use_lap=True):
        out = orig[0](cost, thresh, use_lap)
        if probe is not None and cost.size:
            probe.dist.append(float(np.abs(cost.astype(np.float64) - thresh).min()))
            if thresh == 0.5:
                probe.second += len(out[0])
        return out

    def iou_distance(a, b):
        cost = orig[3](a, b)
        if probe is not None and cost.size:
            ra = np.ascontiguousarray([t.xywha for t in a], dtype=np.float32)
            rb = np.ascontiguousarray([t.xywha for t in b], dtype=np.float32)
            p64 = probiou64(ra, rb)
            sel = (p64 >= 0.1) & (p64 <= 0.97)
            if sel.any():
                probe.err = max(probe.err, float(np.abs(cost.astype(np.float64) - (1 - p64))[sel].max()))
                probe.pairs += int(sel.sum())
        return cost

    def dup(a, b):
        ra, rb = orig[1](a, b)
        if probe is not None:
            pd = orig[3](a, b)
            if pd.size:
                probe.dist.append(float(np.abs(pd.astype(np.float64) - 0.15).min()))
            probe.dups += (len(a) - len(ra)) + (len(b) - len(rb))
        return ra, rb

    def re_activate(self, *a, **k):
        if probe is not None:
            probe.refound += 1
        return orig[2](self, *a, **k)

    matching.linear_assignment, matching.iou_distance = la, iou_distance
    bt.matching = matching
    bt.BYTETracker.remove_duplicate_stracks = staticmethod(dup)
    bt.STrack.re_activate = re_activate
    if float64:
        matching.batch_probiou = lambda a, b: torch.from_numpy(probiou64(a, b))
    try:
        tracker = bt.BYTETracker(IterableSimpleNamespace(tracker_type="bytetrack", **cfg), frame_rate=30)
        outs = []
        for rows in frames:
            if probe is not None:
                for t in (cfg["track_high_thresh"], cfg["track_low_thresh"], cfg["new_track_thresh"]):
                    d = np.abs(rows[:, 5].astype(np.float64) - float(np.float32(t)))
                    d = d[rows[:, 5] != np.float32(t)]
                    if d.size:
                        probe.score_margin = min(probe.score_margin, float(d.min()))
            if len(rows) == 0:  # trackers/track.py:79-80
                outs.append(np.zeros((0, 9), dtype=np.float32))
                continue
            t = tracker.update(SimpleNamespace(xywhr=rows[:, :5], conf=rows[:, 5], cls=rows[:, 6]), None)
            t = np.asarray(t, dtype=np.float32).reshape(-1, 9)
            outs.append(t[np.argsort(t[:, 5], kind="stable")])
        return outs
    finally:
        matching.linear_assignment, bt.BYTETracker.remove_duplicate_stracks, bt.STrack.re_activate, matching.iou_distance, matching.batch_probiou = orig


def run_hull(frames, cfg):
    """The IoU-on-hull answer: this repository's axis-aligned host tracker on the hulls; per frame {idx: id}."""
    from drone_yolo_amd.trackers import ByteTracker

    tr = ByteTracker(dict(cfg, tracker_type="bytetrack"))
    out = []
    for rows in frames:
        r = tr.update(hull_rows(rows)) if len(rows) else np.zeros((0, 8), dtype=np.float32)
        out.append({int(i): int(t) for i, t in zip(r[:, 7], r[:, 4])})
    return out


def record(name, first_seed=1, tries=400):
    for seed in range(first_seed, first_seed + tries):
        frames, cfg = make(name, seed)
        probe = Probe()
        G.FORMULATION[0] = "extended"
        a = run_reference(frames, cfg, probe)
        hull = run_hull(frames, cfg)
        ours = [{int(i): int(t) for i, t in zip(o[:, 8], o[:, 5])} for o in a]
        hull_differs = sum(h != o for h, o in zip(hull, ours))
        margin = max(8 * probe.err, M_FLOOR)
        nearest = min(probe.dist, default=float("inf"))
        ok = {}
        if name == "turning":
            ok["the hull tracker gives other ids"] = hull_differs > 0
            ok["aspect >= 4 throughout"] = all((np.maximum(r[:, 2], r[:, 3]) >= 4 * np.minimum(r[:, 2], r[:, 3])).all() for r in frames)
            th = np.concatenate([r[:, 4] for r in frames])
            ok["angles on both sides of the wrap"] = bool((th < 0.1).any() and (th > math.pi / 2 - 0.1).any())
        ok["no cost within M of its threshold"] = nearest >= margin
        ok["score margin >= 1e-6"] = probe.score_margin >= 1e-6
        if all(ok.values()):
            b64 = run_reference(frames, cfg, float64=True)
            ok["float64 ProbIoU gives the same ids and idx"] = all(x.shape == y.shape and np.array_equal(x[:, [5, 8]], y[:, [5, 8]]) for x, y in zip(a, b64))
        if all(ok.values()):
            G.FORMULATION[0] = "private-dummy"
            b = run_reference(frames, cfg)
            G.FORMULATION[0] = "extended"
            ok["two formulations agree"] = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
        if name == "flicker":
            ok["a re-found track"], ok["a duplicate removal"] = probe.refound > 0, probe.dups > 0
        if name == "sparse":
            ok["a second-stage match"] = probe.second > 0
        if all(ok.values()):
            print(f"{name}: seed {seed}; frames {len(frames)}, detections per frame {min(map(len, frames))}..{max(map(len, frames))}, "
                  f"rows out {sum(map(len, a))}, ids up to {int(max((o[:, 5].max() for o in a if len(o)), default=0))}; M {margin:.2e} "
                  f"(max |cost32 - cost64| {probe.err:.2e} over {probe.pairs} pairs), nearest cost {nearest:.2e}, score margin {probe.score_margin:.2e}, "
                  f"re-found {probe.refound}, duplicates removed {probe.dups}, second-stage matches {probe.second}, frames where the hull tracker "
                  f"differs {hull_differs}; asserted: {', '.join(ok)}")
            return frames, cfg, a, seed, margin
        print(f"{name}: seed {seed} rejected ({', '.join(k for k, v in ok.items() if not v)})")
    raise SystemExit(f"{name}: no seed in {tries} met the conditions")


def main() -> None:
    G.install_lap()
    from oracle.make_golden import import_reference

    import_reference()
    out = {"names": np.array(NAMES), "setting_keys": np.array(G.SETTING_KEYS), "orig_shape": np.array(IMG)}
    for name in NAMES:
        frames, cfg, res, seed, margin = record(name)
        nmax, kmax = max(max(map(len, frames)), 1), max(max(map(len, res)), 1)
        rows, outp = np.zeros((len(frames), nmax, 7), dtype=np.float32), np.zeros((len(frames), kmax, 9), dtype=np.float32)
        for f, (r, o) in enumerate(zip(frames, res)):
            rows[f, : len(r)], outp[f, : len(o)] = r, o
        out[f"{name}_rows"], out[f"{name}_counts"] = rows, np.array([len(r) for r in frames], dtype=np.int32)
        out[f"{name}_out"], out[f"{name}_out_counts"] = outp, np.array([len(o) for o in res], dtype=np.int32)
        out[f"{name}_settings"] = np.array([float(cfg[k]) for k in G.SETTING_KEYS[:-1]] + [30.0], dtype=np.float64)
        out[f"{name}_seed"], out[f"{name}_margin"] = np.array(seed), np.array(margin)
    dst = ROOT / "tests" / "golden" / "track_obb.npz"
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({dst.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
