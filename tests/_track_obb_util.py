"""Helpers of the oriented-box tracking tests (not collected): the sequences of tests/golden/track_obb.npz (tools/make_track_obb_golden.py),
the comparison against the reference's nine-column rows, the hulls an IoU tracker would see, and the seeded random rotated sequences of the
device-against-host test."""
import math

import numpy as np

from tests._util import golden

ULPS = 4  # tests/_track_util.py's bar: the output is rounded to float32 and the reference's `initiate` is partly float32
# the seeds of random_sequence that tests/test_track_obb_gpu.py runs; tests/test_track_obb_host.py asserts that every one keeps the margin
GPU_SEEDS = (5, 6, 7, 11, 15, 17)  # 5 and 15 have a frame without detections; 11 and 15 pass 200 detections


def sequences():
    g = golden("track_obb.npz")
    keys = [str(k) for k in g["setting_keys"]]
    out = {}
    for name in (str(n) for n in g["names"]):
        s = dict(zip(keys, g[f"{name}_settings"].tolist()))
        cfg = dict(tracker_type="bytetrack", track_high_thresh=s["track_high_thresh"], track_low_thresh=s["track_low_thresh"],
                   new_track_thresh=s["new_track_thresh"], track_buffer=int(s["track_buffer"]), match_thresh=s["match_thresh"], fuse_score=bool(s["fuse_score"]))
        out[name] = dict(cfg=cfg, frame_rate=int(s["frame_rate"]), rows=g[f"{name}_rows"], counts=g[f"{name}_counts"], out=g[f"{name}_out"],
                         out_counts=g[f"{name}_out_counts"], margin=float(g[f"{name}_margin"]), seed=int(g[f"{name}_seed"]))
    return out


def margin_all(seq) -> float:
    """M of the random sequences: the largest margin the recording tool measured on any fixture sequence (8 x the float32 error of a cost)."""
    return max(s["margin"] for s in seq.values())


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_rows_match(got, exp, where):
    """Same row count; id, score, cls, idx and the ANGLE equal (the angle bit for bit); x, y, w, h within ULPS float32 ulps of the expected value."""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    assert got.shape == exp.shape and got.shape[1] == 9, f"{where}: rows of shape {got.shape}, expected {exp.shape}"
    assert np.array_equal(got[:, 5], exp[:, 5]), f"{where}: ids {got[:, 5]} != {exp[:, 5]}"
    assert np.array_equal(got[:, 7:], exp[:, 7:]), f"{where}: cls / idx differ"
    assert np.array_equal(got[:, 6], exp[:, 6]), f"{where}: scores differ"
    assert same_bits(got[:, 4], exp[:, 4]), f"{where}: angles differ"
    tol = ULPS * np.spacing(np.abs(exp[:, :4]))
    err = np.abs(got[:, :4].astype(np.float64) - exp[:, :4].astype(np.float64))
    assert (err <= tol).all(), f"{where}: box off by {float((err / np.maximum(tol / ULPS, 1e-45)).max()):.1f} ulps"


def hull_rows(rows):
    """(n, 7) xywhr rows -> (n, 6) [x1, y1, x2, y2, conf, cls]: the axis-aligned hull of the four corners."""
    x, y, w, h, t = (rows[:, k].astype(np.float64) for k in range(5))
    c, s = np.cos(t), np.sin(t)
    ex, ey = np.abs(w / 2 * c) + np.abs(h / 2 * s), np.abs(w / 2 * s) + np.abs(h / 2 * c)
    return np.stack([x - ex, y - ey, x + ex, y + ey, rows[:, 5], rows[:, 6]], axis=1).astype(np.float32)


def random_sequence(seed, frames=10, max_n=300, n_cls=2):
    """10 frames with 0..300 oriented detections: objects drifting and turning over a 1280 x 720 image, aspects 1..8, angles over
    (-pi / 4, 3 pi / 4) as the OBB head emits them, a random subset seen per frame, rows [x, y, w, h, r, conf, cls] in descending score."""
    rng = np.random.default_rng(7000 + seed)
    n_obj = int(rng.integers(20, max_n + 1))
    c = np.stack([rng.uniform(20, 1260, n_obj), rng.uniform(20, 700, n_obj)], axis=1)
    v = rng.uniform(-5, 5, (n_obj, 2))
    length = rng.uniform(24, 90, n_obj)
    wh = np.stack([length, length / rng.uniform(1, 8, n_obj)], axis=1)
    th = rng.uniform(-math.pi / 4, 3 * math.pi / 4, n_obj)
    om = rng.uniform(-0.05, 0.05, n_obj)
    cls = rng.integers(0, n_cls, n_obj)
    out = []
    for f in range(frames):
        p_seen = 0.0 if (seed % 5 == 0 and f == 3) else rng.uniform(0.5, 1.0)
        seen = np.nonzero(rng.random(n_obj) < p_seen)[0]
        p = c[seen] + v[seen] * f + rng.normal(0, 0.7, (len(seen), 2))
        s = wh[seen] * (1 + rng.normal(0, 0.02, (len(seen), 2)))
        t = th[seen] + om[seen] * f + rng.normal(0, 0.01, len(seen))
        t = (t + math.pi / 4) % math.pi - math.pi / 4
        rows = np.concatenate([p, s, t[:, None], rng.uniform(0.05, 0.99, (len(seen), 1)), cls[seen, None]], axis=1).astype(np.float32)
        out.append(rows[np.argsort(-rows[:, 5], kind="stable")])
    return out
