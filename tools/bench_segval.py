"""Times SegmentationValidator.__call__ with the mask matching on the device (dy_val_mask_match) and on the host (GPU box).
usage: python tools/bench_segval.py [--images 16] [--imgsz 640] [--batch 8] [--scale s] [--dtype f16x2] [--labels 12] [--runs 2] [--rounds 2]

The P2 segmentation model (prototype grid imgsz / 2, label map imgsz / 4) with seeded weights; the images live on the device, the labels
and the overlap maps are built from the model's own detections (the `--labels` highest-scored rows of a single-label NMS; their masks
painted into the map, later rows over earlier ones), so that matches exist.  `--mode both` (default) starts one fresh child process per
mode and round, alternating device / host; a child runs one warm-up validation (weight packing, workspaces) and then `--runs` timed
ones, each from the call to its returned dict (which ends in a device-to-host copy, so nothing is left in flight).  The parent commit
cannot validate a segmentation model: the host restatement of the reference's data flow (device_match=False) is the comparison.
Prints one JSON line."""
import argparse, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--scale", default="s")
ap.add_argument("--dtype", default="f16x2", help="storage type of the model pass (cfg/default.yaml: dtype)")
ap.add_argument("--labels", type=int, default=12, help="labels per image (the model's highest-scored detections)")
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--mode", default="both", choices=["both", "device", "host"])
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()

if a.mode == "both":  # the parent never opens the device: one fresh child per (round, mode)
    res = {"device": [], "host": []}
    dicts = {}
    for _ in range(a.rounds):
        for m in ("device", "host"):
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", m] + [f"--{k}={getattr(a, k)}" for k in ("images", "imgsz", "batch", "scale", "dtype", "labels", "runs", "seed")]
            line = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
            r = json.loads(line)
            res[m] += r["ms"]
            dicts[m] = r["metrics"]
            info = {k: r[k] for k in ("labels_total", "rows_kept")}
    print(json.dumps(dict(images=a.images, imgsz=a.imgsz, batch=a.batch, scale=a.scale, dtype=a.dtype, runs=a.runs, rounds=a.rounds, **info,
                          device_ms=res["device"], host_ms=res["host"], device_range=[min(res["device"]), max(res["device"])],
                          host_range=[min(res["host"]), max(res["host"])], disjoint=max(res["device"]) < min(res["host"]) or max(res["host"]) < min(res["device"]),
                          dicts_equal=dicts["device"] == dicts["host"], metrics=dicts["device"])))
    sys.exit(0)

import numpy as np
import torch
import drone_yolo_amd as D
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine.predictor import resolve_dtype
from drone_yolo_amd.engine.trainer import TensorLoader
from drone_yolo_amd.engine.validator import SegmentationValidator, host_pred_masks
from drone_yolo_amd.nn.tasks import SegmentationModel
from drone_yolo_amd.utils import ops
from drone_yolo_amd.utils.parity import seeded_state_dict

dev = torch.device("cuda", 0)
dtype = resolve_dtype(a.dtype)
nc, s = 10, a.imgsz
model = SegmentationModel(f"yolov8{a.scale}-p2-repvgg-seg.yaml", nc=nc, verbose=False)
model.load_state_dict(seeded_state_dict(model.state_dict(), 5, cls_bias=-1.2))
model = model.to(dev).eval()
img = torch.randint(0, 256, (a.images, 3, s, s), generator=torch.Generator().manual_seed(a.seed), dtype=torch.uint8).to(dev)

bi, cls, bb, maps = [], [], [], []
det = model.model[-1]
fuse_tail = getattr(det, "fuse_tail", False)
for s0 in range(0, a.images, a.batch):
    with torch.no_grad():
        det.fuse_tail = False
        y, (_, _, p) = model._predict_once((img[s0 : s0 + a.batch].float() / 255.0).contiguous(), image_dtype=dtype)
        y = y.float().contiguous()
        bufs = ops.non_max_suppression(y, 0.01, 0.7, nc=nc, max_det=a.labels, return_padded=True)
        side = H.mask_gather(bufs, pred=y, nc=nc)
    counts, rows, side, p = bufs.count.cpu().tolist(), bufs.out.cpu(), side.cpu(), p.float().cpu().contiguous()
    for j, k in enumerate(counts):
        gm = torch.zeros((p.shape[2] // 2, p.shape[3] // 2), dtype=torch.uint8)
        pm = host_pred_masks(p[j], side[j, :k, 4:], side[j, :k, :4], (s, s)).bool()[:, ::2, ::2]
        for l in range(k):
            gm[pm[l]] = l + 1
        xyxy = rows[j, :k, :4].clamp(0, s)
        bi.append(torch.full((k,), float(s0 + j))), cls.append(rows[j, :k, 5:6]), maps.append(gm)
        bb.append(torch.stack(((xyxy[:, 0] + xyxy[:, 2]) / 2 / s, (xyxy[:, 1] + xyxy[:, 3]) / 2 / s, (xyxy[:, 2] - xyxy[:, 0]) / s, (xyxy[:, 3] - xyxy[:, 1]) / s), 1))
det.fuse_tail = fuse_tail
data = dict(img=img, batch_idx=torch.cat(bi), cls=torch.cat(cls), bboxes=torch.cat(bb), masks=torch.stack(maps))


def validate():
    v = SegmentationValidator(dict(iou=0.7, max_det=300, device_match=(a.mode == "device")))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = v(model, TensorLoader(data, a.batch, 0, 1, shuffle=False), dev, dtype)
    return time.perf_counter() - t0, out, int(np.sum(v.last_counts))


_, metrics, kept = validate()  # warm-up
ms = [round(validate()[0] * 1e3, 2) for _ in range(a.runs)]
print(json.dumps(dict(mode=a.mode, ms=ms, metrics=metrics, labels_total=int(len(data["cls"])), rows_kept=kept)))
