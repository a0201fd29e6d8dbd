"""Writes tests/golden/track.npz: what the REAL reference's ``BYTETracker`` returns on synthetic detection sequences, for
tests/test_track_host.py and tests/test_track_gpu.py.

    python tools/make_track_golden.py

The reference is imported through oracle/make_golden.py::import_reference (nothing under oracle/ changes).  Its trackers/utils/matching.py
wants the ``lap`` package and would try to install it when the import fails, so a stand-in ``lap`` module goes into ``sys.modules`` BEFORE
anything under ``ultralytics.trackers`` is imported: ``lapjv(cost, extend_cost=True, cost_limit=t)`` solves the extended (n + m)^2 matrix
(off-blocks t / 2, corner 0) with scipy — the problem lap solves; lap's own choice among equal optima is therefore not pinned.  The
reference's ``BYTETracker`` then runs unmodified on ``Boxes(rows, orig_shape)`` built with the reference's own class.

Every sequence is recorded twice, the second time with another exact formulation of the assignment (rectangular, one private dummy column
per row, rows reversed); the tool asserts, per sequence, that the two give identical outputs, that no cost entering a threshold comparison
(match_thresh, 0.5, 0.7, 0.15) lies within 1e-5 of it and that no score lies within 1e-6 of a score threshold unless it equals it; plus the
events each sequence is there for.  When a condition fails the next seed is tried; the conditions are never loosened.  Only arrays go into
the file: per sequence the padded detection rows and counts, the settings, and the reference's rows per frame sorted by track id.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

DEFAULTS = dict(track_high_thresh=0.25, track_low_thresh=0.1, new_track_thresh=0.25, track_buffer=30, match_thresh=0.8, fuse_score=True)
SETTING_KEYS = ("track_high_thresh", "track_low_thresh", "new_track_thresh", "track_buffer", "match_thresh", "fuse_score", "frame_rate")
IMG = (720, 1280)  # orig_shape (h, w)
FORMULATION = ["extended"]


def _solve(cost: np.ndarray, limit: float):
    from scipy.optimize import linear_sum_assignment

    n, m = cost.shape
    c = np.asarray(cost, dtype=np.float64)
    x, y = np.full(n, -1, dtype=np.int64), np.full(m, -1, dtype=np.int64)
    if FORMULATION[0] == "extended":
        e = np.full((n + m, n + m), limit / 2.0)
        e[:n, :m] = c
        e[n:, m:] = 0.0
        r, k = linear_sum_assignment(e)
        for i, j in zip(r, k):
            if i < n and j < m:
                x[i], y[j] = j, i
    else:  # rows reversed, one private dummy column per row at cost `limit`
        big = 1e9
        e = np.full((n, m + n), big)
        e[:, :m] = c[::-1]
        e[np.arange(n), m + np.arange(n)] = limit
        r, k = linear_sum_assignment(e)
        for i, j in zip(r, k):
            if j < m:
                x[n - 1 - i], y[j] = j, n - 1 - i
    total = float(sum(c[i, x[i]] for i in range(n) if x[i] >= 0))
    return total, x, y


def install_lap() -> None:
    lap = types.ModuleType("lap")
    lap.__version__ = "0.5.12"

    def lapjv(cost, extend_cost=False, cost_limit=np.inf, return_cost=True):
        assert extend_cost and np.isfinite(cost_limit)
        return _solve(cost, float(cost_limit))

    lap.lapjv = lapjv
    sys.modules["lap"] = lap


# ---- synthetic scenes ------------------------------------------------------------------------------------
def scene(rng, n_obj, frames, area, size, speed, jitter, p_visible=0.9, n_cls=2, lanes=0, vanish=None, scores=(0.05, 0.98)):
    """Constant-velocity boxes + jitter.  Returns per frame an (n, 6) float32 array in random order."""
    x0, y0, x1, y1 = area
    c = np.stack([rng.uniform(x0, x1, n_obj), rng.uniform(y0, y1, n_obj)], axis=1)
    v = rng.uniform(-speed, speed, (n_obj, 2))
    wh = rng.uniform(size[0], size[1], (n_obj, 2))
    if lanes:  # same size, same direction, small speed differences: objects overtake one another along a few lines
        c[:, 1] = y0 + (y1 - y0) * (rng.integers(0, lanes, n_obj) + 0.5) / lanes
        v[:, 1] = 0
        v[:, 0] = speed + rng.uniform(-2.0, 2.0, n_obj)
        wh[:] = size[0]
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
            j = rng.normal(0, jitter, 4)
            w, h = wh[k] * (1 + 0.02 * j[2:])
            bx = [p[0] + j[0] - w / 2, p[1] + j[1] - h / 2, p[0] + j[0] + w / 2, p[1] + j[1] + h / 2]
            bx = [min(max(bx[0], 0), IMG[1]), min(max(bx[1], 0), IMG[0]), min(max(bx[2], 0), IMG[1]), min(max(bx[3], 0), IMG[0])]
            if bx[2] - bx[0] < 2 or bx[3] - bx[1] < 2:
                continue
            s = rng.uniform(*scores) if rng.random() < 0.3 else rng.uniform(0.5, 0.98)
            rows.append(bx + [s, cls[k]])
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, 6)
        rows = rows[np.argsort(-rows[:, 4], kind="stable")]  # as the NMS leaves them
        out.append(rows)
    return out


def make(name, seed):
    rng = np.random.default_rng(seed)
    cfg = dict(DEFAULTS)
    if name == "sparse":
        fr = scene(rng, 12, 40, (100, 100, 1100, 600), (30, 90), 6, 0.8, p_visible=0.9, n_cls=3)
    elif name == "crowd":
        fr = scene(rng, 150, 12, (500, 260, 780, 460), (40, 80), 3, 0.8, p_visible=0.95, n_cls=2)
    elif name == "flicker":
        cfg["track_buffer"] = 4
        fr = scene(rng, 30, 40, (40, 200, 500, 520), (40, 40), 9, 0.3, n_cls=1, lanes=3, vanish=0.12, scores=(0.26, 0.98))
    elif name == "thresholds":
        fr = scene(rng, 14, 16, (100, 100, 1100, 600), (30, 90), 5, 0.8, p_visible=0.95, n_cls=2)
        special = [np.float32(0.25), np.float32(0.1), np.float32(0.25), np.float32(0.1), np.float32(0.2499), np.float32(0.1001)]
        for f, rows in enumerate(fr):
            if f == 9:  # a frame where every score is low
                rows[:, 4] = rng.uniform(0.11, 0.24, len(rows)).astype(np.float32)
            for k in range(min(len(rows), 4)):
                rows[(3 * k + f) % len(rows), 4] = special[(f + k) % len(special)]
    elif name == "gaps":
        fr = scene(rng, 10, 24, (100, 100, 1100, 600), (30, 90), 6, 0.8, p_visible=0.92, n_cls=2)
        for f in (0, 5, 6, 13, 23):
            fr[f] = np.zeros((0, 6), dtype=np.float32)
    else:
        raise KeyError(name)
    return fr, cfg


# ---- recording ---------------------------------------------------------------------------------------------
class Probe:
    def __init__(self):
        self.cost_margin = self.score_margin = float("inf")
        self.refound = self.dups = self.second = 0


def run_reference(frames, cfg, probe=None):
    from ultralytics.engine.results import Boxes
    from ultralytics.trackers import byte_tracker as bt
    from ultralytics.trackers.utils import matching
    from ultralytics.utils import IterableSimpleNamespace

    orig_la, orig_dup, orig_re = matching.linear_assignment, bt.BYTETracker.remove_duplicate_stracks, bt.STrack.re_activate

    def la(cost, thresh, use_lap=True):
        out = orig_la(cost, thresh, use_lap)
        if probe is not None and cost.size:
            probe.cost_margin = min(probe.cost_margin, float(np.abs(cost.astype(np.float64) - thresh).min()))
            if thresh == 0.5:
                probe.second += len(out[0])
        return out

    def dup(a, b):
        ra, rb = orig_dup(a, b)
        if probe is not None:
            pd = matching.iou_distance(a, b)
            if pd.size:
                probe.cost_margin = min(probe.cost_margin, float(np.abs(pd.astype(np.float64) - 0.15).min()))
            probe.dups += (len(a) - len(ra)) + (len(b) - len(rb))
        return ra, rb

    def re_activate(self, *a, **k):
        if probe is not None:
            probe.refound += 1
        return orig_re(self, *a, **k)

    matching.linear_assignment = la
    bt.BYTETracker.remove_duplicate_stracks = staticmethod(dup)
    bt.STrack.re_activate = re_activate
    try:
        tracker = bt.BYTETracker(IterableSimpleNamespace(tracker_type="bytetrack", **cfg), frame_rate=30)
        outs = []
        for rows in frames:
            if probe is not None:
                for t in (cfg["track_high_thresh"], cfg["track_low_thresh"], cfg["new_track_thresh"]):
                    d = np.abs(rows[:, 4].astype(np.float64) - float(np.float32(t)))
                    d = d[rows[:, 4] != np.float32(t)]
                    if d.size:
                        probe.score_margin = min(probe.score_margin, float(d.min()))
            if len(rows) == 0:  # trackers/track.py:79-80
                outs.append(np.zeros((0, 8), dtype=np.float32))
                continue
            t = tracker.update(Boxes(rows, IMG).numpy(), None)
            t = np.asarray(t, dtype=np.float32).reshape(-1, 8)
            outs.append(t[np.argsort(t[:, 4], kind="stable")])
        return outs
    finally:
        matching.linear_assignment, bt.BYTETracker.remove_duplicate_stracks, bt.STrack.re_activate = orig_la, orig_dup, orig_re


def record(name, first_seed=1, tries=400):
    for seed in range(first_seed, first_seed + tries):
        frames, cfg = make(name, seed)
        probe = Probe()
        FORMULATION[0] = "extended"
        a = run_reference(frames, cfg, probe)
        FORMULATION[0] = "private-dummy"
        b = run_reference(frames, cfg)
        FORMULATION[0] = "extended"
        ok = {
            "two formulations agree": all(np.array_equal(x, y) for x, y in zip(a, b)),
            "cost margin >= 1e-5": probe.cost_margin >= 1e-5,
            "score margin >= 1e-6": probe.score_margin >= 1e-6,
        }
        if name == "flicker":
            ok["a re-found track"], ok["a duplicate removal"] = probe.refound > 0, probe.dups > 0
        if name == "sparse":
            ok["a second-stage match"] = probe.second > 0
        if all(ok.values()):
            print(f"{name}: seed {seed}; frames {len(frames)}, detections per frame {min(map(len, frames))}..{max(map(len, frames))}, "
                  f"rows out {sum(map(len, a))}, ids up to {int(max((o[:, 4].max() for o in a if len(o)), default=0))}; cost margin "
                  f"{probe.cost_margin:.2e}, score margin {probe.score_margin:.2e}, re-found {probe.refound}, duplicates removed {probe.dups}, "
                  f"second-stage matches {probe.second}; asserted: {', '.join(ok)}")
            return frames, cfg, a
        print(f"{name}: seed {seed} rejected ({', '.join(k for k, v in ok.items() if not v)})")
    raise SystemExit(f"{name}: no seed in {tries} met the conditions")


def main() -> None:
    install_lap()
    from oracle.make_golden import import_reference

    import_reference()
    out = {"names": np.array(["sparse", "crowd", "flicker", "thresholds", "gaps"]), "setting_keys": np.array(SETTING_KEYS), "orig_shape": np.array(IMG)}
    for name in out["names"]:
        frames, cfg, res = record(str(name))
        nmax, kmax = max(max(map(len, frames)), 1), max(max(map(len, res)), 1)
        rows, outp = np.zeros((len(frames), nmax, 6), dtype=np.float32), np.zeros((len(frames), kmax, 8), dtype=np.float32)
        for f, (r, o) in enumerate(zip(frames, res)):
            rows[f, : len(r)], outp[f, : len(o)] = r, o
        out[f"{name}_rows"], out[f"{name}_counts"] = rows, np.array([len(r) for r in frames], dtype=np.int32)
        out[f"{name}_out"], out[f"{name}_out_counts"] = outp, np.array([len(o) for o in res], dtype=np.int32)
        out[f"{name}_settings"] = np.array([float(cfg[k]) for k in SETTING_KEYS[:-1]] + [30.0], dtype=np.float64)
    dst = ROOT / "tests" / "golden" / "track.npz"
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({dst.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
