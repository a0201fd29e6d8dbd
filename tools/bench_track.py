"""Times the tracker step (GPU box): dy_track_step on the device, the host path on the same inputs, and the model pass beside them.
usage: python tools/bench_track.py [--steps 8] [--launches 5] [--scale s] [--imgsz 640] [--dtype bf16] [--no-model] [--obb] [--streams 1,16,256]

For S in {1, 16, 256} streams and n in {30, 150, 300} detections per frame: every stream is a scene of n objects drifting over a
1280 x 720 frame (constant velocity + jitter, 95 % seen per frame, scores 0.05 .. 0.99), so that tracks are born, matched, lost and
re-found.  The device figure is one launch of `--steps` time steps (F = steps, all S streams), timed with events after three warm-up
launches, divided by the steps: ms per step for ALL S streams.  The host figure is ByteTracker (numpy, float64) on stream 0's frames,
ms per step of ONE stream, and that times S (the host path walks the streams one after the other).  "model" is the recorded model pass
(Drone-YOLO of `--scale`, `--dtype`, NMS included) at batch S, ms per batch = per step of S streams.  Prints one JSON line.

`--obb`: the same scenes as oriented boxes (every object gets an aspect of 1 .. 8, an angle and a turn rate; rows [x, y, w, h, r, conf, cls])
through dy_track_step_rotated and the host path with rotated=True; the axis-aligned step on the same scenes (the unrotated boxes) is timed
beside it as `axis_device_ms_per_step`."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--launches", type=int, default=5)
ap.add_argument("--scale", default="s")
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--no-model", action="store_true")
ap.add_argument("--obb", action="store_true")
ap.add_argument("--streams", default="1,16,256")
a = ap.parse_args()
dev = torch.device("cuda", 0)

from drone_yolo_amd.trackers import ByteTracker, DeviceByteTracker

MAX_DET = 300


def scene(seed, n, frames, obb=False):
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(20, 1260, n), rng.uniform(20, 700, n)], axis=1)
    v, wh = rng.uniform(-5, 5, (n, 2)), rng.uniform(16, 70, (n, 2))
    if obb:
        wh[:, 1] = wh[:, 0] / rng.uniform(1, 8, n)
        th, om = rng.uniform(-np.pi / 4, 3 * np.pi / 4, n), rng.uniform(-0.05, 0.05, n)
    rows = np.zeros((frames, MAX_DET, 7 if obb else 6), dtype=np.float32)
    counts = np.zeros(frames, dtype=np.int32)
    for f in range(frames):
        seen = np.nonzero(rng.random(n) < 0.95)[0]
        p = c[seen] + v[seen] * f + rng.normal(0, 0.7, (len(seen), 2))
        conf, cls = rng.uniform(0.05, 0.99, (len(seen), 1)), np.zeros((len(seen), 1))
        if obb:
            t = (th[seen] + om[seen] * f + np.pi / 4) % np.pi - np.pi / 4
            r = np.concatenate([p, wh[seen], t[:, None], conf, cls], axis=1).astype(np.float32)
        else:
            r = np.concatenate([p - wh[seen] / 2, p + wh[seen] / 2, conf, cls], axis=1).astype(np.float32)
        r = r[np.argsort(-r[:, -2], kind="stable")]
        rows[f, : len(r)], counts[f] = r, len(r)
    return rows, counts


def unrotated(rows):
    """(.., 7) xywhr rows -> (.., 6) xyxy rows of the same centres and sizes: what the axis-aligned step is timed on beside the rotated one."""
    xy, wh = rows[..., :2], rows[..., 2:4]
    return np.ascontiguousarray(np.concatenate([xy - wh / 2, xy + wh / 2, rows[..., 5:7]], axis=-1))


def time_device(tr, rows_d, counts_d, step):
    times = []
    for k in range(3 + a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o, c = tr.update_batch(rows_d[k * step : (k + 1) * step], counts_d[k * step : (k + 1) * step])
        e1.record()
        torch.cuda.synchronize()
        if k >= 3:
            times.append(e0.elapsed_time(e1) / a.steps)
    return times, float(c.float().mean())


out = {"steps_per_launch": a.steps, "obb": a.obb, "grid": []}
W = 7 if a.obb else 6
STREAMS = tuple(int(v) for v in a.streams.split(","))
total = (3 + a.launches) * a.steps
for S in STREAMS:
    for n in (30, 150, 300):
        per = [scene(1000 * S + 10 * n + k % 16, n, total, a.obb) for k in range(min(S, 16))]  # 16 distinct scenes, repeated over the streams
        rows = np.stack([per[k % len(per)][0] for k in range(S)], axis=1).reshape(total * S, MAX_DET, W)  # image f * S + k = stream k at step f
        counts = np.stack([per[k % len(per)][1] for k in range(S)], axis=1).reshape(total * S)
        rows_d, counts_d = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev)
        tr = DeviceByteTracker(streams=S, max_det=MAX_DET, device=dev, rotated=a.obb)
        step = a.steps * S
        times, tracks = time_device(tr, rows_d, counts_d, step)
        axis = None
        if a.obb:
            axis, _ = time_device(DeviceByteTracker(streams=S, max_det=MAX_DET, device=dev), torch.from_numpy(unrotated(rows)).to(dev), counts_d, step)
        host = ByteTracker(max_det=MAX_DET, rotated=a.obb)
        hr, hc = per[0]
        for f in range(3 * a.steps):
            host.update(hr[f, : hc[f]])
        t0 = time.perf_counter()
        for f in range(3 * a.steps, total):
            host.update(hr[f, : hc[f]])
        host_ms = (time.perf_counter() - t0) * 1e3 / (total - 3 * a.steps)
        out["grid"].append({"streams": S, "detections": n, "tracks_out": round(tracks, 1), "device_ms_per_step": round(float(np.median(times)), 4),
                            "device_ms_min_max": [round(min(times), 4), round(max(times), 4)], "host_ms_per_step_one_stream": round(host_ms, 3),
                            "host_ms_per_step_all_streams": round(host_ms * S, 2), "overflow": int(tr.overflow.sum())})
        if axis is not None:
            out["grid"][-1].update({"axis_device_ms_per_step": round(float(np.median(axis)), 4), "axis_device_ms_min_max": [round(min(axis), 4), round(max(axis), 4)]})
        print(json.dumps(out["grid"][-1]), file=sys.stderr, flush=True)

if not a.no_model:
    import drone_yolo_amd as D
    from drone_yolo_amd.engine.predictor import DetectionPredictor, resolve_dtype
    from drone_yolo_amd.utils.parity import seeded_state_dict

    model = D.DetectionModel(f"yolov8{a.scale}-p2-repvgg.yaml", nc=10, verbose=False)
    model.load_state_dict(seeded_state_dict(model.state_dict(), 5, cls_bias=-1.2))
    pred = DetectionPredictor(model, dict(conf=0.1, iou=0.7, dtype=resolve_dtype(a.dtype), device=0))
    out["model"] = []
    for S in STREAMS:
        x = torch.rand(S, 3, a.imgsz, a.imgsz, generator=torch.Generator().manual_seed(S)).to(dev)
        for _ in range(3):
            pred.forward_device(x)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pred.forward_device(x)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        out["model"].append({"batch": S, "ms_per_batch": round(float(np.median(ts)), 3), "ms_per_image": round(float(np.median(ts)) / S, 4)})
print(json.dumps(out))
