"""Times YOLO.val of an oriented-box model with the matching on the device (dy_val_match_rotated) and on the host, and the two kernels of
the validator's post-processing on their own (GPU box).
usage: python tools/bench_obbval.py [--images 16] [--imgsz 640] [--batch 8] [--scale s] [--dtype f16x2] [--labels 12] [--runs 5] [--rounds 2]
       python tools/bench_obbval.py --mode kernels

The P2 oriented-box model with seeded weights; the images live on the device, the labels are built from the model's own detections (the
`--labels` highest-scored rows of the single-label rotated NMS), so that matches exist.  `--mode both` (default) starts one fresh child
process per mode and round, alternating device / host; a child runs one warm-up validation (weight packing, workspaces) and then `--runs`
timed ones, each from the call of YOLO.val to its returned dict (which ends in a device-to-host copy, so nothing is left in flight).  The
parent commit cannot validate an oriented-box model: the host restatement of the reference's data flow (device_match=False) is the
comparison.  `--mode kernels`: per batch, the device time (events, median of `--runs` after a warm-up) of the validator's NMS call
(hip_ops.nms_rotated_ml at conf 0.001: the counter reset, nms_filter_ml_kernel and nms_rotated_ml_kernel) and of the matching call
(hip_ops.val_match_rotated: the label padding and val_match_rotated_kernel), next to the candidate counts per image.  Prints one JSON line."""
import argparse, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--scale", default="s")
ap.add_argument("--dtype", default="f16x2", help="storage type of the model pass (cfg/default.yaml: dtype)")
ap.add_argument("--labels", type=int, default=12, help="labels per image (the model's highest-scored detections)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--mode", default="both", choices=["both", "device", "host", "kernels"])
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
from drone_yolo_amd.engine.validator import OBBValidator, obb_labels
from drone_yolo_amd.nn.tasks import OBBModel
from drone_yolo_amd.utils.parity import seeded_state_dict

dev = torch.device("cuda", 0)
dtype = resolve_dtype(a.dtype)
nc, s = 10, a.imgsz
yolo = D.YOLO(f"yolov8{a.scale}-p2-repvgg-obb.yaml")
yolo.model = OBBModel(f"yolov8{a.scale}-p2-repvgg-obb.yaml", nc=nc, verbose=False)  # (the YAML's own nc is 80)
yolo.model.load_state_dict(seeded_state_dict(yolo.model.state_dict(), 5, cls_bias=-1.2))
assert yolo.model.yaml["nc"] == nc
model = yolo.model.to(dev).eval()
img = torch.randint(0, 256, (a.images, 3, s, s), generator=torch.Generator().manual_seed(a.seed), dtype=torch.uint8).to(dev)


def passes():
    """(y, theta) of every batch through the validator's own model pass."""
    det = model.model[-1]
    fuse_tail = getattr(det, "fuse_tail", False)
    out = []
    for s0 in range(0, a.images, a.batch):
        with torch.no_grad():
            det.fuse_tail = False
            y, _ = model._predict_once((img[s0 : s0 + a.batch].float() / 255.0).contiguous(), image_dtype=dtype)
        y = y.float()
        out.append((y[:, : 4 + nc].contiguous(), y[:, -1].contiguous()))
    det.fuse_tail = fuse_tail
    return out


bi, cls, bb = [], [], []
batches = passes()
for n0, (y, th) in enumerate(batches):
    bufs = H.nms_rotated(y, th, 0.01, 0.7, max_det=a.labels, nc=nc)
    counts, rows = bufs.count.cpu().tolist(), bufs.out.cpu()
    for j, k in enumerate(counts):
        r = rows[j, :k]
        bi.append(torch.full((k,), float(n0 * a.batch + j))), cls.append(r[:, 6:7])
        bb.append(torch.stack((r[:, 0] / s, r[:, 1] / s, r[:, 2] / s, r[:, 3] / s, r[:, 4]), 1))
data = dict(img=img, batch_idx=torch.cat(bi), cls=torch.cat(cls), bboxes=torch.cat(bb))

if a.mode == "kernels":
    lim = torch.tensor((s, s, s, s), dtype=torch.float32, device=dev)
    iouv = np.linspace(0.5, 0.95, 10)
    per_batch = []
    for n0, (y, th) in enumerate(batches):
        sel = (data["batch_idx"] >= n0 * a.batch) & (data["batch_idx"] < (n0 + 1) * a.batch)
        tbox = obb_labels(data["bboxes"][sel].to(dev), s, s, lim)
        tcls, timg = data["cls"][sel].view(-1).to(dev), (data["batch_idx"][sel] - n0 * a.batch).to(torch.int32).to(dev)
        bufs = H.nms_rotated_ml(y, th, 0.001, 0.7, max_det=300, nc=nc)  # warm-up
        H.val_match_rotated(bufs, tbox, tcls, timg, iouv, (s, s))
        torch.cuda.synchronize()
        cand = bufs.workspace[: 4 * y.shape[0]].view(torch.int32).cpu().tolist()  # the candidate counters at the head of the workspace
        t_nms, t_match = [], []
        for _ in range(a.runs):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            H.nms_rotated_ml(y, th, 0.001, 0.7, max_det=300, nc=nc, bufs=bufs)
            e[1].record()
            H.val_match_rotated(bufs, tbox, tcls, timg, iouv, (s, s))
            e[2].record()
            torch.cuda.synchronize()
            t_nms.append(e[0].elapsed_time(e[1])), t_match.append(e[1].elapsed_time(e[2]))
        per_batch.append(dict(candidates=cand, kept=bufs.count.cpu().tolist(), labels=int(sel.sum()), nms_ms=round(float(np.median(t_nms)), 3),
                              nms_ms_range=[round(min(t_nms), 3), round(max(t_nms), 3)], match_ms=round(float(np.median(t_match)), 3),
                              match_ms_range=[round(min(t_match), 3), round(max(t_match), 3)]))
    print(json.dumps(dict(mode="kernels", images=a.images, imgsz=a.imgsz, batch=a.batch, scale=a.scale, dtype=a.dtype, anchors=int(batches[0][0].shape[2]), nc=nc,
                          runs=a.runs, batches=per_batch)))
    sys.exit(0)


def validate():
    kept = []

    def make(args):
        kept.append(OBBValidator(args))
        return kept[0]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = yolo.val(validator=make, data=data, batch=a.batch, dtype=a.dtype, iou=0.7, max_det=300, device=0, device_match=(a.mode == "device"))
    return time.perf_counter() - t0, out, int(np.sum(kept[0].last_counts))


_, metrics, kept = validate()  # warm-up
ms = [round(validate()[0] * 1e3, 2) for _ in range(a.runs)]
print(json.dumps(dict(mode=a.mode, ms=ms, metrics=metrics, labels_total=int(len(data["cls"])), rows_kept=kept)))
