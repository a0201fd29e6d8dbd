"""Times the pose path (GPU box): a pose model's pass beside its detection twin, and `predict(frames, crops=...)` against the list-of-crops call.
usage: python tools/bench_pose.py [--rounds 7] [--scale s] [--dtype float16] [--imgsz 640] [--batch 16] [--crops 8,32,128] [--crop-batch 32]

A and B alternate in one process after warm-up; each figure is the median over `--rounds` rounds with the smallest and largest beside it.
  (a) pass    one batch of `--batch` images at imgsz^2: host clock around predict() (results built) and device time of the recorded pass, for
              yolov8<scale>-p2-repvgg-pose.yaml and its detection twin yolov8<scale>-p2-repvgg.yaml (nc 1 both).  The difference is the keypoint
              branches, dy_kpt_decode (gather form) and dy_scale_coords.
  (b) crops   per crop count k: k person boxes spread over two 4K frames (2160 x 3840 uint8), person-sized (60-200 px wide, 2-3 times as tall).
              A = predict([frame[y0:y1, x0:x1] ...], imgsz, batch): the host cuts each window and the predictor letterboxes them one by one;
              B = predict(frames, crops=boxes, imgsz, batch): one upload of the frames, one slicer launch per batch.  Host clock around the whole
              call, crops per second.  Both upload from host memory: B the two frames (50 MB), A the windows.
  (c) slicer  dy_crops_letterbox_u8_to_nchw_f32 alone on k crops already on the device: ms, and GB/s of the bytes it writes (12 per output pixel).
Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--scale", default="s")
ap.add_argument("--dtype", default="float16")
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--crops", default="8,32,128")
ap.add_argument("--crop-batch", type=int, default=32)
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/bench_pose.py needs an MI355X"
dev = torch.device("cuda", 0)

from drone_yolo_amd import YOLO
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine import crops as CR


def stat(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def model(name):
    y = YOLO(name)
    if y.model.yaml["nc"] != 1:
        from drone_yolo_amd.nn.tasks import DetectionModel, yaml_model_load

        y.model = DetectionModel(yaml_model_load(name), nc=1, verbose=False)
    for m in y.model.model[-1].cv3:  # stock bias leaves no candidates: lift the class bias so that rows survive
        m[-1].bias.data += 8.0
    return y


res = {"scale": a.scale, "dtype": a.dtype, "imgsz": a.imgsz, "rounds": a.rounds, "pass": {}, "crops": [], "slicer": []}
gen = torch.Generator().manual_seed(3)
x = torch.rand(a.batch, 3, a.imgsz, a.imgsz, generator=gen).to(dev)
kw = dict(device=0, dtype=a.dtype, conf=0.25, iou=0.7)
ys = {"pose": model(f"yolov8{a.scale}-p2-repvgg-pose.yaml"), "detect": model(f"yolov8{a.scale}-p2-repvgg.yaml")}
for y in ys.values():
    for _ in range(3):
        y.predict(x, **kw)
torch.cuda.synchronize()
host, devt = {k: [] for k in ys}, {k: [] for k in ys}
for _ in range(a.rounds):
    for k, y in ys.items():
        host[k].append(host_ms(lambda: y.predict(x, **kw)))
        devt[k].append(timed(lambda: y.predictor.forward_device(x)))
for k, y in ys.items():
    p = y.predictor
    r = y.predict(x, **kw)
    res["pass"][k] = {"batch": a.batch, "predict_ms": stat(host[k]), "recorded_pass_ms": stat(devt[k]), "rows_per_image": round(float(np.mean([len(q) for q in r])), 1),
                      "launches": len(p._compiled[next(iter(p._compiled))].plan.ops)}

rng = np.random.default_rng(5)
frames = rng.integers(0, 256, (2, 2160, 3840, 3), dtype=np.uint8)
pose = ys["pose"]
ckw = dict(kw, imgsz=a.imgsz, batch=a.crop_batch, crop_expand=0.2)  # (the same arguments for both calls: one predictor, one set of recorded passes)
for k in [int(v) for v in a.crops.split(",")]:
    boxes = [[], []]
    for j in range(k):
        w = float(rng.uniform(60, 200))
        h = w * float(rng.uniform(2.0, 3.0))
        x0, y0 = float(rng.uniform(0, 3840 - w)), float(rng.uniform(0, 2160 - h))
        boxes[j % 2].append([x0, y0, x0 + w, y0 + h])
    boxes = [np.array(b, dtype=np.float32).reshape(-1, 4) for b in boxes]
    rects = CR.crop_rects(list(frames), boxes, 0.2)

    def run_list():
        return pose.predict([np.ascontiguousarray(frames[f, y0:y1, x0:x1]) for f, x0, y0, x1, y1 in rects], **ckw)

    def run_crops():
        return pose.predict(frames, crops=boxes, **ckw)

    for _ in range(2):
        run_list(), run_crops()
    ts = {"list_of_crops": [], "crops": []}
    for _ in range(a.rounds):
        ts["list_of_crops"].append(host_ms(run_list))
        ts["crops"].append(host_ms(run_crops))
    res["crops"].append({"crops": k, "batch": a.crop_batch, "ms": {n: stat(v) for n, v in ts.items()},
                         "crops_per_s": {n: stat([k / (t * 1e-3) for t in v]) for n, v in ts.items()}})
    fd = torch.from_numpy(frames).to(dev)
    table = torch.from_numpy(CR.crop_table(rects, a.imgsz))
    td = table.to(dev)
    out = torch.empty((k, 3, a.imgsz, a.imgsz), dtype=torch.float32, device=dev)
    H.crops_letterbox(fd, table, a.imgsz, a.imgsz, out=out, table_dev=td)
    t = [timed(lambda: H.crops_letterbox(fd, table, a.imgsz, a.imgsz, out=out, table_dev=td)) for _ in range(a.rounds)]
    wrote = k * 3 * a.imgsz * a.imgsz * 4
    res["slicer"].append({"crops": k, "ms": stat(t), "bytes_written": wrote, "GBps": round(wrote / (float(np.median(t)) * 1e-3) / 1e9, 1)})
    del fd, out
print(json.dumps(res))
