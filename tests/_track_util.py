"""Helpers of the tracking tests (not collected): the sequences of tests/golden/track.npz, the comparison against the reference's rows
and the seeded random sequences of the device-against-host test."""
import numpy as np

from tests._util import golden

ULPS = 4  # the output is rounded to float32 and the reference's `initiate` is partly float32; a logic error moves a box by thousands of ulps


def sequences():
    g = golden("track.npz")
    keys = [str(k) for k in g["setting_keys"]]
    out = {}
    for name in (str(n) for n in g["names"]):
        s = dict(zip(keys, g[f"{name}_settings"].tolist()))
        cfg = dict(tracker_type="bytetrack", track_high_thresh=s["track_high_thresh"], track_low_thresh=s["track_low_thresh"],
                   new_track_thresh=s["new_track_thresh"], track_buffer=int(s["track_buffer"]), match_thresh=s["match_thresh"], fuse_score=bool(s["fuse_score"]))
        out[name] = dict(cfg=cfg, frame_rate=int(s["frame_rate"]), rows=g[f"{name}_rows"], counts=g[f"{name}_counts"], out=g[f"{name}_out"],
                         out_counts=g[f"{name}_out_counts"])
    return out


def assert_rows_match(got, exp, where):
    """Same row count; id, cls, idx and score equal; boxes within ULPS float32 ulps of the expected value."""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    assert got.shape == exp.shape, f"{where}: {got.shape[0]} rows, expected {exp.shape[0]}"
    assert np.array_equal(got[:, 4], exp[:, 4]), f"{where}: ids {got[:, 4]} != {exp[:, 4]}"
    assert np.array_equal(got[:, 6:], exp[:, 6:]), f"{where}: cls / idx differ"
    assert np.array_equal(got[:, 5], exp[:, 5]), f"{where}: scores differ"
    tol = ULPS * np.spacing(np.abs(exp[:, :4]))
    err = np.abs(got[:, :4].astype(np.float64) - exp[:, :4].astype(np.float64))
    assert (err <= tol).all(), f"{where}: box off by {float((err / np.maximum(tol / ULPS, 1e-45)).max()):.1f} ulps"


def random_sequence(seed, frames=10, max_n=300, n_cls=2):
    """10 frames with 0..300 detections: objects drifting over a 1280 x 720 image, a random subset seen per frame, rows in descending score."""
    rng = np.random.default_rng(1000 + seed)
    n_obj = int(rng.integers(20, max_n + 1))
    c = np.stack([rng.uniform(20, 1260, n_obj), rng.uniform(20, 700, n_obj)], axis=1)
    v = rng.uniform(-5, 5, (n_obj, 2))
    wh = rng.uniform(16, 70, (n_obj, 2))
    cls = rng.integers(0, n_cls, n_obj)
    out = []
    for f in range(frames):
        p_seen = 0.0 if (seed % 5 == 0 and f == 3) else rng.uniform(0.5, 1.0)
        seen = np.nonzero(rng.random(n_obj) < p_seen)[0]
        p = c[seen] + v[seen] * f + rng.normal(0, 0.7, (len(seen), 2))
        s = wh[seen] * (1 + rng.normal(0, 0.02, (len(seen), 2)))
        rows = np.concatenate([p - s / 2, p + s / 2, rng.uniform(0.05, 0.99, (len(seen), 1)), cls[seen, None]], axis=1).astype(np.float32)
        out.append(rows[np.argsort(-rows[:, 4], kind="stable")])
    return out
