"""Times DetectionValidator.__call__ with the host match and with the device match (GPU box).
usage: python tools/bench_val.py [--images 512] [--imgsz 640] [--batch 64] [--scale s] [--dtype bf16] [--labels 70] [--runs 5]

A synthetic tensor dataset whose images live on the device (the labels stay where TensorLoader indexes them, on the host): Drone-YOLO
of the given scale with seeded weights, labels = the model's own detections, `--labels` per image on average from a skewed draw (some
images carry several hundred), so that matches exist.  After one warm-up validation per mode the modes alternate; every validation is
timed from the call to its returned dict (which ends in a device-to-host copy, so nothing is left in flight).  "model" is a loop of its
own over the same loader that does only the image conversion, the model pass and the validation loss; "outside" = whole - median model.
Run from a checkout without `device_match` (the parent of the commit that added it) the script times the host match alone: that is the
baseline.  Prints one JSON line."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import drone_yolo_amd as D
from drone_yolo_amd.engine.predictor import resolve_dtype
from drone_yolo_amd.engine.trainer import TensorLoader
from drone_yolo_amd.engine.validator import DetectionValidator
from drone_yolo_amd.utils import ops
from drone_yolo_amd.utils.parity import seeded_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=512)
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--scale", default="s")
ap.add_argument("--dtype", default="bf16", help="storage type of the model pass (cfg/default.yaml: dtype)")
ap.add_argument("--labels", type=float, default=70.0, help="labels per image on average")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
dev = torch.device("cuda", 0)
dtype = resolve_dtype(a.dtype)
nc, s = 10, a.imgsz
model = D.DetectionModel(f"yolov8{a.scale}-p2-repvgg.yaml", nc=nc, verbose=False)
model.load_state_dict(seeded_state_dict(model.state_dict(), 5, cls_bias=-1.2))
model = model.to(dev).eval()
g = torch.Generator().manual_seed(a.seed)
img = torch.randint(0, 256, (a.images, 3, s, s), generator=g, dtype=torch.uint8).to(dev)

# labels: per image the n best of the model's own detections (single-label NMS at a low threshold), n from a lognormal draw
rng = np.random.default_rng(a.seed)
want = np.minimum(rng.lognormal(np.log(a.labels) - 0.5, 1.0, a.images).astype(int), 600)
bi, cls, bb = [], [], []
det = model.model[-1]
fuse_tail = getattr(det, "fuse_tail", False)
for s0 in range(0, a.images, a.batch):
    with torch.no_grad():
        det.fuse_tail = False
        y, _ = model._predict_once((img[s0 : s0 + a.batch].float() / 255.0).contiguous(), image_dtype=dtype)
        dets = ops.non_max_suppression(y, 0.01, 0.7, nc=nc, max_det=600)
    for j, d in enumerate(dets):
        d = d[: want[s0 + j]].cpu()
        xyxy = d[:, :4].clamp(0, s)
        bi.append(torch.full((len(d),), float(s0 + j))), cls.append(d[:, 5:6])
        bb.append(torch.stack(((xyxy[:, 0] + xyxy[:, 2]) / 2 / s, (xyxy[:, 1] + xyxy[:, 3]) / 2 / s, (xyxy[:, 2] - xyxy[:, 0]) / s, (xyxy[:, 3] - xyxy[:, 1]) / s), 1))
det.fuse_tail = fuse_tail
data = dict(img=img, batch_idx=torch.cat(bi), cls=torch.cat(cls), bboxes=torch.cat(bb))
per_img = np.bincount(data["batch_idx"].long().numpy(), minlength=a.images)

has_device = DetectionValidator(dict(device_match=True)).__dict__.get("device_match", False)
modes = ["host", "device"] if has_device else ["host"]


def validate(mode):
    v = DetectionValidator(dict(iou=0.7, max_det=300, device_match=(mode == "device")))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = v(model, TensorLoader(data, a.batch, 0, 1, shuffle=False), dev, dtype)
    return time.perf_counter() - t0, out


def model_only():
    loss = torch.zeros(3, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for batch in TensorLoader(data, a.batch, 0, 1, shuffle=False):
        x = batch["img"].to(dev).float() / 255.0
        with torch.no_grad():
            det.fuse_tail = False
            y, feats = model._predict_once(x.contiguous(), image_dtype=dtype)
            loss += model.criterion(feats, batch)[1]
    loss.cpu()
    det.fuse_tail = fuse_tail
    return time.perf_counter() - t0


results = {m: validate(m)[1] for m in modes}  # warm-up (weight packing, workspaces) and the dicts to compare
times = {m: [] for m in modes}
model_t = []
for _ in range(a.runs):
    for m in modes:
        times[m].append(validate(m)[0])
    model_t.append(model_only())
med_model = statistics.median(model_t)
out = dict(images=a.images, imgsz=s, batch=a.batch, scale=a.scale, dtype=str(dtype), labels_mean=float(per_img.mean()), labels_max=int(per_img.max()),
           runs=a.runs, model_ms=[round(t * 1e3, 2) for t in model_t], mAP50=results["host"]["metrics/mAP50(B)"])
for m in modes:
    out[f"{m}_ms"] = [round(t * 1e3, 2) for t in times[m]]
    out[f"{m}_outside_ms"] = [round((t - med_model) * 1e3, 2) for t in times[m]]
if has_device:
    out["dicts_equal"] = results["host"] == results["device"]
print(json.dumps(out))
